// mcmc_colorer_amd/csrc/chains_tailcut16.h -- the corrected tail cut of a half-word chain batch (nCol up to 2048).
//
// Included by chains.hip inside namespace mcmc::{anonymous}, after chains_wide16.h and chains_tailcut.h.
// The contract is chains_tailcut.h's (chain r ends as the oracle's run with tailcutRepair and its own
// nCol, epsilon, seed); the list kernel, the row walker (tail_row_chunks), TailArgs, TailMasks and the
// host's pass loop are the byte path's. What reads a colour is new, because a colour is a uint16_t here
// (C16[buffer][group][v][64]) and a chain's occupancy is up to 64 words:
//
//   chains_tail_normalise16_kernel  thread k takes the 8-byte word k of the group's n x 16 (chains
//       4 (k & 15) .. +3 of vertex k >> 4) and copies the half-words of the chains that stopped in
//       buffer 1 into buffer 0 (mask_halves: sel4 for half-words); the first n threads also write the
//       first pass's flag word (w0 & ~pm) | (w1 & pm).
//   chains_tail_count16_kernel<TILED>  the recount on the half-word sweep's grid (wide16_waves(MW) waves
//       per workgroup, vb vertices per wave) with its load shape: lane (q = l >> 4, i = l & 15) loads the
//       8-byte word of chains 4 i .. 4 i + 3 of neighbour q of a step's four, 512 B per wave-load, eight
//       in flight. A lane keeps the row's own word; zero_halves(w ^ own) is exact and carry-free; hits
//       are OR-reduced over the quarters and the row's scan ends once every chain still being repaired
//       has hit. Output as the byte kernel's: the flag word per (group, v), per-chain counts.
//   chains_tail_repair16_kernel<TILED, MW>  walks the group's ascending union list; only the lanes
//       flagged at v write. A walk is a serial chain of memory round trips per vertex, and the single
//       run's repair walks only its own ~100 flagged vertices, so one workgroup walking the union of
//       64 chains cannot beat 64 single runs (measured: 152 to 198 ms against 72 ms). Chains are
//       independent -- chain l's pass reads and writes only chain l's colours -- so kTail16Subs = 64
//       workgroups per group run at once, each owning one chain: per tile of 1024 list entries it
//       keeps, in order, the vertices at which its chain is flagged (ballot + wave totals, as the list
//       kernel) and walks those. It loads the group's whole 128-byte colour rows as every kernel here
//       does and ORs all 64 columns; the other chains' half-words may be mid-pass in another
//       workgroup, and are never read back from the table. 16 waves put a row of up to 1024
//       neighbours in flight at once (one 64-neighbour chunk each, 16 loads per lane). The groups'
//       changed words are ORed atomically; the host clears them before the launch.
//       Occupancy: one shared LDS table occ[MW][64] (4, 8 or 16 KB), cleared per vertex up to the words
//       the largest nCol under repair uses. The waves split the row's 64-neighbour chunks; a loaded word
//       is rotated right by 16 q, so that half-word j is chain 4 i + ((j + q) & 3) and each of a step's
//       four ds_or_b32 addresses 64 distinct columns. The OR does not return and nothing is counted: the
//       repair needs the first free colour, not Zv.
//       Colour order: a chain's colorIdx is up to 2048 half-words, 256 KB for a group -- not LDS. It
//       lives in global memory, one row per chain: cidx16[group * 64 + l][ncmax]. A lane that walks
//       its own row pays one L2 round trip per few steps, and at 300 colours and degree 1000 the first
//       free colour lies deep in the order (the first version did that: 194 ms for the first pass of
//       the ladder 300:363 on G(1e5, 0.01)). So wave 0 walks cooperatively: for each chain flagged at v
//       (mostly one) its 64 lanes test positions k0 .. k0 + 255 of that chain's row at once -- four
//       coalesced 128-byte loads, the colour's bit read from the chain's LDS column, a ballot per 64
//       positions in ascending order -- so a whole 256-colour stretch of the order costs one round
//       trip. The chain's lane takes the colour found, its own when none is free, and stores the
//       half-word. With the identity order (no tailcut: z = 0) the table is neither built nor read:
//       the first clear bit is the count of trailing zeros of the first nonzero ~occ word of the
//       column, bounded by nCol.
//       Visibility, prefetch of the next listed vertex and its row_off pair, the per-group "changed"
//       word and the zeroing of the counts: exactly chains_tail_repair_kernel's. Colour loads of a pass
//       are agent-scope atomic loads (served from L2), every wave issues __threadfence() before the
//       barrier that ends a vertex. Plain C++ / HIP atomics and vector stores only.
//
// Resources (hipcc -O3 -ffp-contract=off, gfx950, -Rpass-analysis=kernel-resource-usage): see DESIGN.md,
// "Half-word batches: the tail cut".
#pragma once

// 0x8000 in every half-word of x that is zero (exact: no carry crosses a half-word)
__device__ __forceinline__ uint64_t zero_halves(uint64_t x) {
    constexpr uint64_t k7 = 0x7FFF7FFF7FFF7FFFull;
    return ~(((x & k7) + k7) | x | k7);
}

// sel4 for half-words: 0xFFFF in half-word j when bit 4 i + j of the group's mask is set
__device__ __forceinline__ uint64_t mask_halves(uint64_t mask, uint32_t i) {
    const uint64_t b = (mask >> (4u * i)) & 15ull;
    return ((b & 1ull) * 0xFFFFull) | ((b & 2ull) * (0xFFFF0000ull >> 1)) | ((b & 4ull) * (0xFFFF00000000ull >> 2)) |
           ((b & 8ull) * (0xFFFF000000000000ull >> 3));
}

// Grid (chunks of 256 words, group): thread k of the grid's x takes 8-byte word k of the group's n x 16;
// the first n threads also take one flag word each.
__global__ __launch_bounds__(256) void chains_tail_normalise16_kernel(ChainArgs a, TailArgs ta, TailMasks buf1, TailMasks par1) {
    const uint32_t g = blockIdx.y, n = a.n;
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t b1 = buf1.m[g], pm = par1.m[g];
    if (k < (uint64_t)n * 16u && b1 != 0ull) {
        const uint64_t sel = mask_halves(b1, (uint32_t)(k & 15u));
        if (sel) {
            uint64_t* W0 = reinterpret_cast<uint64_t*>(a.C[0]) + (size_t)g * n * 16u;
            const uint64_t* W1 = reinterpret_cast<const uint64_t*>(a.C[1]) + (size_t)g * n * 16u;
            W0[k] = (W0[k] & ~sel) | (W1[k] & sel);
        }
    }
    if (k < n) {
        const uint64_t* f0 = a.vfl + (size_t)g * n, *f1 = a.vfl + ((size_t)a.G + g) * n;
        ta.fl[(size_t)g * n + k] = (f0[k] & ~pm) | (f1[k] & pm);
    }
}

// K steps of a chunk's recount: K 8-byte loads issued, then K half-word-wise compares with the row's own word
template <int K>
__device__ __forceinline__ uint64_t count16_steps(const uint64_t* __restrict__ Cq, uint32_t cur, uint32_t s0, uint32_t rem,
                                                  uint32_t q, uint32_t i, uint32_t nlast, uint64_t own) {
    uint64_t w[K], h = 0ull;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nlast);
        w[k] = Cq[(size_t)id * 16u + i];
    }
#pragma unroll
    for (int k = 0; k < K; k++) h |= zero_halves(w[k] ^ own);
    return h;
}

// Launched with the half-word sweep's workgroup: blockDim.x / 64 = wide16_waves(MW) waves.
template <bool TILED>
__global__ __launch_bounds__(64 * kSweepWaves) void chains_tail_count16_kernel(ChainArgs a, TailArgs ta, TailMasks act) {
    __shared__ uint32_t s_cnt[kLanes];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t waves = blockDim.x >> 6;
    const uint32_t g = blockIdx.y, n = a.n;
    const uint64_t am = act.m[g];
    if (am == 0ull) return;   // workgroup-uniform
    if (threadIdx.x < kLanes) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t v0l = ((uint64_t)blockIdx.x * waves + wid) * a.vb;
    const uint32_t v1 = (uint32_t)min((uint64_t)n, v0l + a.vb);
    const uint64_t* __restrict__ Cq = reinterpret_cast<const uint64_t*>(a.C[0]) + (size_t)g * n * 16u;
    const uint64_t act4 = mask_halves(am, i) & 0x8000800080008000ull;
    const bool mine = (am >> lane) & 1ull;
    uint32_t cnt = 0u;
    for (uint64_t vl = v0l; vl < v1; vl++) {
        const uint32_t v = (uint32_t)vl;
        const uint64_t own = Cq[(size_t)v * 16u + i];
        uint64_t base = 0, deg = 0;
        if constexpr (!TILED) {
            const uint64_t end = min(a.row_off[v + 1], a.m);
            base = min(a.row_off[v], end);
            deg = end - base;
        }
        uint64_t h = 0ull;
        tail_row_chunks<TILED>(a, v, base, deg, lane, 0u, 1u, [&](uint32_t cur, uint32_t rem) {
            for (uint32_t s = 0; 4u * s < rem;) {
                if (rem - 4u * s > 16u) {
                    h |= count16_steps<8>(Cq, cur, s, rem, q, i, n - 1u, own);
                    s += 8u;
                } else {
                    h |= count16_steps<4>(Cq, cur, s, rem, q, i, n - 1u, own);
                    s += 4u;
                }
            }
            h = or_xor64(or_xor64(h, 16), 32);
            return (bool)__all((h & act4) == act4);
        });
        // chain `lane`: half-word lane & 3 of lane lane >> 2
        const uint64_t hv = shfl64(h, (int)(lane >> 2));
        const bool hit = mine && ((hv >> (16u * (lane & 3u) + 15u)) & 1ull);
        const uint64_t fb = __ballot(hit);
        if (lane == 0u) ta.fl[(size_t)g * n + v] = fb;
        cnt += hit ? 1u : 0u;
    }
    if (cnt) atomicAdd(&s_cnt[lane], cnt);
    __syncthreads();
    if (threadIdx.x < kLanes && s_cnt[threadIdx.x]) atomicAdd(&ta.cnt[g * kLanes + threadIdx.x], s_cnt[threadIdx.x]);
}

// K steps of a chunk of the repair: K 8-byte loads that see this pass's stores, then K x 4 ORs into the
// workgroup's table. colp[j]: word 0 of the column of chain 4 i + ((j + q) & 3); rot = 16 q.
template <int K, int MW>
__device__ __forceinline__ void repair16_steps(const uint64_t* Cq, uint32_t cur, uint32_t s0, uint32_t rem, uint32_t q,
                                               uint32_t i, uint32_t nlast, uint32_t rot, uint32_t* const (&colp)[4]) {
    uint64_t w[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nlast);
        w[k] = __hip_atomic_load(Cq + (size_t)id * 16u + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint64_t wr = (w[k] >> rot) | (w[k] << ((64u - rot) & 63u));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c = (uint32_t)(wr >> (16 * j)) & 0xFFFFu;
            // rows past MW - 1 folded back: a colour is below its chain's nCol <= 32 MW
            (void)__hip_atomic_fetch_or(colp[j] + ((c >> 5) & (uint32_t)(MW - 1)) * kLanes, 1u << (c & 31u), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

constexpr uint32_t kTail16Waves = 16;   // waves of the half-word repair workgroup
constexpr uint32_t kTail16Subs = 64;    // repair workgroups per group: each owns 64 / kTail16Subs chains

// MW: words of a chain's occupancy column, the batch's (16, 32 or 64). One workgroup per group.
// ncmax: entries per chain of the colour-order table (the batch's largest nCol).
template <bool TILED, int MW>
__global__ __launch_bounds__(64 * kTail16Waves) void chains_tail_repair16_kernel(ChainArgs a, TailArgs ta, TailMasks act,
                                                                               uint32_t ncmax) {
    __shared__ uint32_t s_occ[MW * kLanes];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t s_sel[64 * kTail16Waves];   // a list tile's vertices that this workgroup's chains visit
    __shared__ uint32_t s_tot[kTail16Waves];
    const uint32_t g = blockIdx.x / kTail16Subs, sub = blockIdx.x % kTail16Subs, n = a.n;
    if (act.m[g] == 0ull) return;   // workgroup-uniform
    // the recount that follows adds to the counts
    if (sub == 0u && threadIdx.x < kLanes) ta.cnt[g * kLanes + threadIdx.x] = 0u;
    const uint64_t am = act.m[g] & (((1ull << (kLanes / kTail16Subs)) - 1ull) << (sub * (kLanes / kTail16Subs)));
    if (am == 0ull) return;         // none of this workgroup's chains is under repair
    const uint32_t L = min(ta.listlen[g], n);
    uint16_t* Ch = reinterpret_cast<uint16_t*>(a.C[0]) + (size_t)g * n * kLanes;
    const uint64_t* Cq = reinterpret_cast<const uint64_t*>(Ch);
    const uint64_t* fl = ta.fl + (size_t)g * n;
    const uint32_t* list = ta.list + (size_t)g * n;
    uint32_t* const colp[4] = {s_occ + 4u * i + (q & 3u), s_occ + 4u * i + ((q + 1u) & 3u),
                               s_occ + 4u * i + ((q + 2u) & 3u), s_occ + 4u * i + ((q + 3u) & 3u)};
    const uint32_t* const mycol = s_occ + lane;
    const uint32_t rot = 16u * q;
    const uint32_t nl = min((uint32_t)a.ncolw[g * kLanes + lane], min(ncmax, 32u * (uint32_t)MW));
    // the table's words in use: those of the largest nCol under repair (every wave computes the same)
    uint32_t nw = ((am >> lane) & 1ull) ? nl : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nw = max(nw, (uint32_t)__shfl_xor((int)nw, o, 64));
    nw = ((uint32_t)__builtin_amdgcn_readfirstlane((int)nw) + 31u) >> 5;
    const bool ident = a.z == 0u;   // colorIdx is the identity: no table
    const uint16_t* ci = reinterpret_cast<const uint16_t*>(ta.cidx) + (size_t)g * kLanes * ncmax;
    bool changed = false;
    for (uint32_t t0 = 0; t0 < L; t0 += 64u * kTail16Waves) {
    // the tile's listed vertices at which a chain of this workgroup is flagged, in the list's order
    uint32_t T = 0u;
    {
        const uint32_t kk = t0 + threadIdx.x;
        const uint32_t vv = kk < L ? min(list[kk], n - 1u) : 0u;
        const bool on = kk < L && (fl[vv] & am) != 0ull;
        const uint64_t b = __ballot(on);
        if (lane == 0u) s_tot[wid] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kTail16Waves; w++) {
            const uint32_t x = s_tot[w];
            before += w < wid ? x : 0u;
            T += x;
        }
        if (on) s_sel[before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = vv;
        __syncthreads();
    }
    // the vertex ahead and (CSR) its row_off pair: loaded during the row before it
    uint32_t vn = T ? s_sel[0] : 0u;
    uint64_t rn0 = 0, rn1 = 0;
    if constexpr (!TILED) {
        rn0 = a.row_off[vn];
        rn1 = a.row_off[vn + 1];
    }
    for (uint32_t k = 0; k < T; k++) {
        const uint32_t v = vn;
        const uint64_t end = min(rn1, a.m), base = min(rn0, end);
        if (k + 1u < T) {
            vn = s_sel[k + 1u];
            if constexpr (!TILED) {
                rn0 = a.row_off[vn];
                rn1 = a.row_off[vn + 1];
            }
        }
        const uint64_t f = fl[v] & am;
        for (uint32_t w = threadIdx.x; w < nw * kLanes; w += 64u * kTail16Waves) s_occ[w] = 0u;
        __syncthreads();
        tail_row_chunks<TILED>(a, v, base, end - base, lane, wid, kTail16Waves, [&](uint32_t cur, uint32_t rem) {
            for (uint32_t s = 0; 4u * s < rem;) {
                if (rem - 4u * s > 32u) {
                    repair16_steps<16, MW>(Cq, cur, s, rem, q, i, n - 1u, rot, colp);
                    s += 16u;
                } else if (rem - 4u * s > 16u) {
                    repair16_steps<8, MW>(Cq, cur, s, rem, q, i, n - 1u, rot, colp);
                    s += 8u;
                } else {
                    repair16_steps<4, MW>(Cq, cur, s, rem, q, i, n - 1u, rot, colp);
                    s += 4u;
                }
            }
            return false;
        });
        __syncthreads();
        if (wid == 0u && f != 0ull) {   // wave-uniform: every thread read the same flag word
            const bool flagged = (f >> lane) & 1ull;
            uint32_t old = 0u;
            if (flagged) old = __hip_atomic_load(Ch + (size_t)v * kLanes + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t newc = old;
            if (ident) {   // the first clear bit of the column below nCol
                for (uint32_t w = 0; flagged && 32u * w < nl; w++) {
                    uint32_t x = ~mycol[w * kLanes];
                    if (nl - 32u * w < 32u) x &= (1u << (nl - 32u * w)) - 1u;
                    if (x) {
                        newc = 32u * w + (uint32_t)__builtin_ctz(x);
                        break;
                    }
                }
            } else {       // per flagged chain: the wave tests 256 positions of its order per round trip
                uint64_t fm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(f >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)f);
                while (fm != 0ull) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(fm);
                    fm &= fm - 1ull;
                    const uint32_t nc = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)nl, (int)l, 64));
                    const uint16_t* row = ci + (size_t)l * ncmax;
                    const uint32_t* col = s_occ + l;
                    bool found = false;
                    uint32_t take = 0u;
                    for (uint32_t k0 = 0; k0 < nc && !found; k0 += 256u) {
                        uint32_t c4[4];
#pragma unroll
                        for (uint32_t j = 0; j < 4u; j++) c4[j] = row[min(k0 + 64u * j + lane, nc - 1u)];
#pragma unroll
                        for (uint32_t j = 0; j < 4u; j++) {
                            const uint32_t c = c4[j];
                            const bool fr = k0 + 64u * j + lane < nc &&
                                            !((col[((c >> 5) & (uint32_t)(MW - 1)) * kLanes] >> (c & 31u)) & 1u);
                            const uint64_t b = __ballot(fr);
                            if (!found && b != 0ull) {   // the lowest position of the lowest 64: the order's first free colour
                                take = (uint32_t)__shfl((int)c, __builtin_ctzll(b), 64);
                                found = true;
                            }
                        }
                    }
                    if (lane == l && found) newc = take;
                }
            }
            if (flagged && newc != old) {
                Ch[(size_t)v * kLanes + lane] = (uint16_t)newc;
                changed = true;
            }
        }
        __threadfence();   // the half-word is in L2 before any wave loads the next row's neighbours
        __syncthreads();   // also: s_sel and s_tot are free for the next tile
    }
    }
    const uint64_t cb = __ballot(changed);
    if (threadIdx.x == 0u && cb != 0ull) atomicOr(reinterpret_cast<unsigned long long*>(ta.chg + g), cb);   // zeroed by the host
}
