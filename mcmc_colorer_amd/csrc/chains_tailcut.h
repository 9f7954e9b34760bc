// mcmc_colorer_amd/csrc/chains_tailcut.h -- the corrected tail cut of a chain batch, 64 chains per row read.
//
// Included by chains.hip inside namespace mcmc::{anonymous}, after ChainArgs, tiled_chunk and the
// sweeps. Chain r ends as oracle/mcmc_cpu_ref.cpp::tail_cut leaves its single run: while its Cviol > 0
// (at most max_passes passes) every flagged vertex, in ascending order, takes the first colour of the
// chain's colorIdx that no neighbour holds (its own when none is free), reading the colours the same
// pass has already written; then Cviol and the flags are recounted. The first pass uses the flags of
// C_{iter-1} (C_0 when iter = 0): the sweeps' FLAGS instantiations keep, per (group, v), the ballot
// of `viol` of sweep t at vfl[t & 1][group][v], merged under the live mask so that a stopped chain
// keeps its bits.
//
// Everything reads the batch's layout as the sweep does: lane l of a wave-load holds the dword of
// chains 4 (l & 15) .. +3 of neighbour l >> 4, 256 B per load and several in flight; rows come from the
// CSR or from the tiled layout's directory rounds and tiled_chunk (tail_row_chunks below).
//
//   chains_tail_normalise_kernel  the chains of a group stop in different buffers: copies every chain's
//       final colouring into buffer 0 (per-byte select, as the histogram kernels) and writes the first
//       pass's flag word (w0 & ~pm) | (w1 & pm), pm = chains whose flag parity is 1. Both masks come from
//       the host, which holds every chain's state at that point; the host then sets buf = 0.
//   chains_tail_list_kernel       per group the ascending list of vertices whose flag word has a bit of
//       a chain still being repaired: one workgroup per group, tiles of 1024 vertices, ballot + wave
//       totals in LDS (double buffered: one barrier per tile). Order preserving by construction.
//   chains_tail_repair_kernel<TILED, MW>  one workgroup per group walks the group's list in order.
//       Chains are independent and each needs only its own flagged vertices in ascending order, so the
//       union list, with only the lanes flagged at v writing, is exact for all 64 chains at once. Per
//       vertex the waves split the row's 64-neighbour chunks and OR colour bits into one shared LDS
//       table occ[MW][64] (ds_or_b32, the wide sweep's rotated dword: 64 distinct columns per
//       instruction); after a barrier lane l of wave 0, if flagged, walks its chain's colorIdx (a byte
//       table staged in LDS, rows padded to 260 bytes: lane l's row starts in bank l) to the first clear
//       bit and stores the byte.
//       Visibility: a pass's colours are loaded with agent-scope atomic loads (they bypass the
//       CU's vector L1, whose lines are not invalidated by another wave's store) and wave 0 issues
//       __threadfence() before the workgroup barrier, so the byte is in L2 -- where those loads are
//       served -- before any wave starts the next vertex. The same rule the single-chain kernel
//       (tailcut.hip: volatile loads + __threadfence) relies on.
//       The next listed vertex and, for CSR rows, its row_off pair are loaded during the current row.
//   chains_tail_count_kernel<TILED>  the recount, one path for narrow and wide batches: the sweep's grid;
//       a lane keeps the row's own dword and compares every neighbour dword byte-wise (exact zero-byte
//       test on w ^ own, carry-free), hits OR-reduced over the quarters (xor 16 / 32); the row's scan
//       ends once every chain still being repaired has hit. Output: the flag word per (group, v) limited
//       to those chains, and per-chain counts (per-lane sum, LDS sum, one atomic per workgroup and chain).
#pragma once

constexpr uint32_t kTailWaves = 4;        // waves of the repair workgroup
constexpr uint32_t kTailListThreads = 1024;
constexpr uint32_t kCidxStride = 260;     // bytes per chain of the staged colorIdx: 65 dwords, bank = chain
constexpr uint32_t kMaxGroups = kMaxChains / kLanes;

struct TailMasks { uint64_t m[kMaxGroups]; };   // one bit per chain, by group

struct TailArgs {
    uint64_t* fl;        // [G][n] the flag words a pass visits
    uint32_t* list;      // [G][n]
    uint32_t* listlen;   // [G]
    uint8_t* cidx;       // [G * 64][256] colorIdx per chain
    uint32_t* cnt;       // [G * 64] violators after the pass; followed by
    uint64_t* chg;       // [G] chains of which the pass changed a byte
};

// 0x80 in every byte of x that is zero (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) {
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// f(cur, rem) for the chunks part, part + parts, ... of 64 ids of row v (lane j: id j, `rem` valid)
// until f returns true (wave-uniform). CSR: base, deg are the row's; the next chunk's ids are in
// flight during f. Tiled: the sweep's directory rounds, chunks counted through the rounds.
template <bool TILED, class F>
__device__ __forceinline__ void tail_row_chunks(const ChainArgs& a, uint32_t v, uint64_t base, uint64_t deg, uint32_t lane,
                                                uint32_t part, uint32_t parts, F&& f) {
    if constexpr (!TILED) {
        uint64_t c0 = 64ull * part;
        uint32_t ids = c0 + lane < deg ? a.col_idx[base + c0 + lane] : 0u;
        for (; c0 < deg; c0 += 64ull * parts) {
            const uint32_t cur = ids;
            const uint64_t nx = c0 + 64ull * parts + lane;
            ids = nx < deg ? a.col_idx[base + nx] : 0u;
            if (f(cur, (uint32_t)min((uint64_t)64u, deg - c0))) return;
        }
    } else {
        const uint32_t grp = v / a.grp_rows, rg = v - grp * a.grp_rows, tstride = tseg_stride(a.grp_rows);
        const uint16_t* __restrict__ ids16 = a.tcol + a.gbase[grp];
        const uint32_t* __restrict__ ts = a.tseg + (size_t)grp * a.nblocks * tstride + rg;
        uint32_t k = 0u;
        for (uint32_t b0 = 0; b0 < a.nblocks; b0 += 64u) {
            uint32_t seg0 = 0u, len = 0u;
            if (b0 + lane < a.nblocks) {
                const uint32_t* ent = ts + (size_t)(b0 + lane) * tstride;
                const uint32_t e0 = ent[0];
                seg0 = e0 & kTsegPos;
                len = (ent[1] & kTsegPos) - seg0 - (e0 & 7u);
            }
            uint32_t endo = len;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)endo, o, 64);
                if (lane >= (uint32_t)o) endo += y;
            }
            const uint32_t delta = seg0 - (endo - len);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)endo, 63);
            for (uint32_t c0 = 0; c0 < total; c0 += 64u, k++) {
                if (k % parts != part) continue;
                const uint32_t cur = tiled_chunk(ids16, delta, endo, c0, total, b0, a.block_log2, lane);
                if (f(cur, min(64u, total - c0))) return;
            }
        }
    }
}

// sel4: 0xFF in byte j when bit 4 i + j of the group's mask is set
__device__ __forceinline__ uint32_t mask_bytes(uint64_t mask, uint32_t i) {
    const uint32_t b = (uint32_t)(mask >> (4u * i)) & 15u;
    return ((b & 1u) * 0xFFu) | ((b & 2u) * (0xFF00u >> 1)) | ((b & 4u) * (0xFF0000u >> 2)) | ((b & 8u) * (0xFF000000u >> 3));
}

// Grid (vertex chunks of 256 * 16 dwords ..., group): thread k of the grid's x takes dword k of the
// group's n x 16; the first n threads also take one flag word each.
__global__ __launch_bounds__(256) void chains_tail_normalise_kernel(ChainArgs a, TailArgs ta, TailMasks buf1, TailMasks par1) {
    const uint32_t g = blockIdx.y, n = a.n;
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t b1 = buf1.m[g], pm = par1.m[g];
    if (k < (uint64_t)n * 16u && b1 != 0ull) {
        const uint32_t sel = mask_bytes(b1, (uint32_t)(k & 15u));
        if (sel) {
            uint32_t* W0 = reinterpret_cast<uint32_t*>(a.C[0] + (size_t)g * n * kLanes);
            const uint32_t* W1 = reinterpret_cast<const uint32_t*>(a.C[1] + (size_t)g * n * kLanes);
            W0[k] = (W0[k] & ~sel) | (W1[k] & sel);
        }
    }
    if (k < n) {
        const uint64_t* f0 = a.vfl + (size_t)g * n, *f1 = a.vfl + ((size_t)a.G + g) * n;
        ta.fl[(size_t)g * n + k] = (f0[k] & ~pm) | (f1[k] & pm);
    }
}

__global__ __launch_bounds__(kTailListThreads) void chains_tail_list_kernel(ChainArgs a, TailArgs ta, TailMasks act) {
    __shared__ uint32_t s_w[2][kTailListThreads / 64u];
    const uint32_t g = blockIdx.x, n = a.n, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t am = act.m[g];
    const uint64_t* __restrict__ fl = ta.fl + (size_t)g * n;
    uint32_t* __restrict__ list = ta.list + (size_t)g * n;
    uint32_t base = 0u, par = 0u;
    for (uint64_t v0 = 0; v0 < n && am != 0ull; v0 += kTailListThreads, par ^= 1u) {
        const uint64_t v = v0 + threadIdx.x;
        const bool on = v < n && (fl[v] & am) != 0ull;
        const uint64_t b = __ballot(on);
        if (lane == 0u) s_w[par][wid] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kTailListThreads / 64u; w++) {
            const uint32_t x = s_w[par][w];
            before += w < wid ? x : 0u;
            total += x;
        }
        if (on) list[base + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)v;
        base += total;
    }
    if (threadIdx.x == 0u) ta.listlen[g] = base;
}

// K steps of a chunk's recount: K loads issued, then K byte-wise compares with the row's own dword
template <int K>
__device__ __forceinline__ uint32_t count_steps(const uint32_t* __restrict__ Cw, uint32_t cur, uint32_t s0, uint32_t rem,
                                                uint32_t q, uint32_t i, uint32_t nlast, uint32_t own) {
    uint32_t w[K], h = 0u;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nlast);
        w[k] = Cw[(size_t)id * 16u + i];
    }
#pragma unroll
    for (int k = 0; k < K; k++) h |= zero_bytes(w[k] ^ own);
    return h;
}

template <bool TILED>
__global__ __launch_bounds__(64 * kSweepWaves) void chains_tail_count_kernel(ChainArgs a, TailArgs ta, TailMasks act) {
    __shared__ uint32_t s_cnt[kLanes];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.y, n = a.n;
    const uint64_t am = act.m[g];
    if (am == 0ull) return;   // workgroup-uniform
    if (threadIdx.x < kLanes) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t v0l = ((uint64_t)blockIdx.x * kSweepWaves + wid) * a.vb;
    const uint32_t v1 = (uint32_t)min((uint64_t)n, v0l + a.vb);
    const uint32_t* __restrict__ Cw = reinterpret_cast<const uint32_t*>(a.C[0] + (size_t)g * n * kLanes);
    const uint32_t act4 = mask_bytes(am, i) & 0x80808080u;
    const bool mine = (am >> lane) & 1ull;
    uint32_t cnt = 0u;
    for (uint64_t vl = v0l; vl < v1; vl++) {
        const uint32_t v = (uint32_t)vl, own = Cw[(size_t)v * 16u + i];
        uint64_t base = 0, deg = 0;
        if constexpr (!TILED) {
            const uint64_t end = min(a.row_off[v + 1], a.m);
            base = min(a.row_off[v], end);
            deg = end - base;
        }
        uint32_t h = 0u;
        tail_row_chunks<TILED>(a, v, base, deg, lane, 0u, 1u, [&](uint32_t cur, uint32_t rem) {
            for (uint32_t s = 0; 4u * s < rem;) {
                if (rem - 4u * s > 16u) {
                    h |= count_steps<8>(Cw, cur, s, rem, q, i, n - 1u, own);
                    s += 8u;
                } else {
                    h |= count_steps<4>(Cw, cur, s, rem, q, i, n - 1u, own);
                    s += 4u;
                }
            }
            h |= (uint32_t)__shfl_xor((int)h, 16, 64);
            h |= (uint32_t)__shfl_xor((int)h, 32, 64);
            return (bool)__all((h & act4) == act4);
        });
        // chain `lane`: byte lane & 3 of lane lane >> 2
        const uint32_t hv = (uint32_t)__shfl((int)h, (int)(lane >> 2), 64);
        const bool hit = mine && ((hv >> (8u * (lane & 3u) + 7u)) & 1u);
        const uint64_t fb = __ballot(hit);
        if (lane == 0u) ta.fl[(size_t)g * n + v] = fb;
        cnt += hit ? 1u : 0u;
    }
    if (cnt) atomicAdd(&s_cnt[lane], cnt);
    __syncthreads();
    if (threadIdx.x < kLanes && s_cnt[threadIdx.x]) atomicAdd(&ta.cnt[g * kLanes + threadIdx.x], s_cnt[threadIdx.x]);
}

// K steps of a chunk of the repair: K loads that see this pass's stores, then K x 4 ORs into the
// workgroup's table. colp[j]: word 0 of the column of chain 4 i + ((j + q) & 3); rot = 8 q.
template <int K, int MW>
__device__ __forceinline__ void repair_steps(const uint32_t* Cw, uint32_t cur, uint32_t s0, uint32_t rem, uint32_t q,
                                             uint32_t i, uint32_t nlast, uint32_t rot, uint32_t* const (&colp)[4]) {
    constexpr uint32_t kRow = (uint32_t)(MW - 1) << 5;
    uint32_t w[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nlast);
        w[k] = __hip_atomic_load(Cw + (size_t)id * 16u + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t wr = __builtin_rotateright32(w[k], rot);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c = (wr >> (8 * j)) & 255u;
            (void)__hip_atomic_fetch_or(colp[j] + (c & kRow) * 2u, 1u << (c & 31u), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// MW: words of a chain's occupancy (4: every nCol of the batch <= 128, else 8). One workgroup per group.
template <bool TILED, int MW>
__global__ __launch_bounds__(64 * kTailWaves) void chains_tail_repair_kernel(ChainArgs a, TailArgs ta, TailMasks act) {
    __shared__ uint32_t s_occ[MW * kLanes];
    __shared__ uint32_t s_cidx[kLanes * kCidxStride / 4u];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.x, n = a.n;
    const uint64_t am = act.m[g];
    if (am == 0ull) return;   // workgroup-uniform
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(ta.cidx) + (size_t)g * kLanes * 64u;
        for (uint32_t k = threadIdx.x; k < kLanes * 64u; k += 64u * kTailWaves)
            s_cidx[(k >> 6) * (kCidxStride / 4u) + (k & 63u)] = src[k];
    }
    if (threadIdx.x < kLanes) ta.cnt[g * kLanes + threadIdx.x] = 0u;   // the recount that follows adds to it
    const uint32_t L = min(ta.listlen[g], n);
    uint8_t* Cb = a.C[0] + (size_t)g * n * kLanes;
    const uint32_t* Cw = reinterpret_cast<const uint32_t*>(Cb);
    const uint64_t* fl = ta.fl + (size_t)g * n;
    const uint32_t* list = ta.list + (size_t)g * n;
    uint32_t* const colp[4] = {s_occ + 4u * i + (q & 3u), s_occ + 4u * i + ((q + 1u) & 3u),
                               s_occ + 4u * i + ((q + 2u) & 3u), s_occ + 4u * i + ((q + 3u) & 3u)};
    const uint32_t rot = 8u * q;
    const uint32_t nl = a.ncolw[g * kLanes + lane];
    const uint8_t* ci = reinterpret_cast<const uint8_t*>(s_cidx) + lane * kCidxStride;
    bool changed = false;
    // the listed vertex ahead and (CSR) its row_off pair: loaded during the row before it
    uint32_t vn = L ? min(list[0], n - 1u) : 0u;
    uint64_t rn0 = 0, rn1 = 0;
    if constexpr (!TILED) {
        rn0 = a.row_off[vn];
        rn1 = a.row_off[vn + 1];
    }
    for (uint32_t k = 0; k < L; k++) {
        const uint32_t v = vn;
        const uint64_t end = min(rn1, a.m), base = min(rn0, end);
        if (k + 1u < L) {
            vn = min(list[k + 1u], n - 1u);
            if constexpr (!TILED) {
                rn0 = a.row_off[vn];
                rn1 = a.row_off[vn + 1];
            }
        }
        const uint64_t f = fl[v] & am;
        for (uint32_t w = threadIdx.x; w < (uint32_t)MW * kLanes; w += 64u * kTailWaves) s_occ[w] = 0u;
        __syncthreads();
        tail_row_chunks<TILED>(a, v, base, end - base, lane, wid, kTailWaves, [&](uint32_t cur, uint32_t rem) {
            for (uint32_t s = 0; 4u * s < rem;) {
                if (rem - 4u * s > 16u) {
                    repair_steps<8, MW>(Cw, cur, s, rem, q, i, n - 1u, rot, colp);
                    s += 8u;
                } else {
                    repair_steps<4, MW>(Cw, cur, s, rem, q, i, n - 1u, rot, colp);
                    s += 4u;
                }
            }
            return false;
        });
        __syncthreads();
        if (wid == 0u && ((f >> lane) & 1ull)) {
            const uint32_t old = __hip_atomic_load(Cb + (size_t)v * kLanes + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t newc = old;
            for (uint32_t j = 0; j < nl; j++) {   // the first colour of colorIdx no neighbour holds
                const uint32_t c = ci[j];
                if (!((s_occ[((c >> 5) & (uint32_t)(MW - 1)) * kLanes + lane] >> (c & 31u)) & 1u)) {
                    newc = c;
                    break;
                }
            }
            if (newc != old) {
                Cb[(size_t)v * kLanes + lane] = (uint8_t)newc;
                changed = true;
            }
        }
        __threadfence();   // the byte is in L2 before any wave loads the next row's neighbours
        __syncthreads();
    }
    const uint64_t cb = __ballot(changed);
    if (threadIdx.x == 0u) ta.chg[g] = cb;
}
