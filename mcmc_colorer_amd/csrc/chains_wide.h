// mcmc_colorer_amd/csrc/chains_wide.h -- the wide sweep of the batched chains: per-lane nCol up to 256.
//
// Included by chains.hip inside namespace mcmc::{anonymous}, after ChainArgs, tiled_chunk and the
// constants. The narrow sweep keeps a lane's occupancy in one 64-bit register pair; here it lives in
// LDS, MW = 4 or 8 words of 32 colours per chain (MW from the batch's largest nCol).
//
// Table: each wave owns occ[MW][64] 32-bit words, column l = chain l of the wave's group, row w =
//   colours 32 w .. 32 w + 31. Nobody but the wave touches it: no workgroup barrier in the row loop.
// Set:  the drain's wave-load is the narrow kernel's (lane (q = l >> 4, i = l & 15) holds the dword of
//   chains 4 i .. 4 i + 3 of neighbour q of the step's four, eight loads in flight). The dword is
//   rotated right by 8 q once, so that byte j of it is chain 4 i + ((j + q) & 3); sub-step j = 0..3
//   issues one ds_or_b32 (no return) of 1 << (c & 31) at row c >> 5 of that chain's column. In one
//   such instruction the 64 lanes address 64 distinct columns ((j + q) & 3 differs over the
//   quarters, 4 i over a quarter), so the four neighbours of a step never meet in a word: no
//   per-quarter copies of the table and no cross-quarter reduction. Slots past the row's end
//   re-read the chunk's first neighbour (OR is idempotent).
// Read: a wave's LDS instructions execute in order; a wave-scope fence and a wave barrier keep the
//   compiler from moving a column's read over the other lanes' ORs. After a chunk of 64 neighbours
//   lane l reads its MW words; the row's scan stops when every live chain's words hold all of ITS
//   colours (word w against full_l[w]; a chain that is not live has full = 0 and counts as full).
//   The test is skipped while fewer neighbours are drained than the wave's smallest live nCol.
// Update: the MW words stay in registers (every word loop is unrolled: static indices, no scratch).
//   Zv is the popcount over them, the own-colour bit comes from word c >> 5, and the CDF walk is the
//   ladder's: fp32, strict `cdf > u`, the single run's addition order, to the wave's largest live
//   nCol in groups of 8 with the wave-wide exit, a lane adding and testing only while k < nCol_l;
//   "not found" is nCol_l. Taboo, the Cn write, the overflow record and the engine step are the
//   narrow kernel's.
#pragma once

// orders the wave's LDS accesses for the compiler (the hardware executes them in order)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// K steps of the drain from step s0 of the chunk whose ids `cur` holds: K loads issued, then K x 4
// ORs into the table. colp[j]: word 0 of the column of chain 4 i + ((j + q) & 3); rot = 8 q.
template <int K, int MW>
__device__ __forceinline__ void drain_steps_wide(const uint32_t* __restrict__ Cw, uint32_t cur, uint32_t s0, uint32_t rem,
                                                 uint32_t q, uint32_t i, uint32_t nlast, uint32_t rot,
                                                 uint32_t* const (&colp)[4]) {
    constexpr uint32_t kRow = (uint32_t)(MW - 1) << 5;   // c & kRow = 32 (c >> 5), rows past MW - 1 folded back
    uint32_t w[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nlast);
        w[k] = Cw[(size_t)id * 16u + i];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t wr = __builtin_rotateright32(w[k], rot);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c = (wr >> (8 * j)) & 255u;
            (void)__hip_atomic_fetch_or(colp[j] + (c & kRow) * 2u, 1u << (c & 31u), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
}

// the 4-neighbour steps over the `rem` ids of `cur`
template <int MW>
__device__ __forceinline__ void drain_chunk_wide(const uint32_t* __restrict__ Cw, uint32_t cur, uint32_t rem, uint32_t q,
                                                 uint32_t i, uint32_t nlast, uint32_t rot, uint32_t* const (&colp)[4]) {
    for (uint32_t s = 0; 4u * s < rem;) {
        if (rem - 4u * s > 16u) {
            drain_steps_wide<8, MW>(Cw, cur, s, rem, q, i, nlast, rot, colp);
            s += 8u;
        } else {
            drain_steps_wide<4, MW>(Cw, cur, s, rem, q, i, nlast, rot, colp);
            s += 4u;
        }
    }
}

// TILED as in chains_sweep_kernel. MW: 32-bit words of a chain's occupancy (4: every nCol <= 128,
// 8: <= 256). Always "ladder style": nCol, epsilon, hi, full, fr, ps and the walk's end are per lane
// (a.ncolw, a.epsr). FLAGS as in chains_sweep_kernel.
template <bool TILED, int MW, bool FLAGS>
__global__ __launch_bounds__(64 * kSweepWaves) void chains_sweep_wide_kernel(ChainArgs a, uint32_t t, uint32_t tn) {
    if (*a.ndone >= a.R) return;   // every chain stopped (workgroup-uniform)
    __shared__ uint32_t s_viol[kLanes];
    __shared__ uint32_t s_occ[kSweepWaves * MW * kLanes];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.y, r = g * kLanes + lane;
    if (threadIdx.x < kLanes) s_viol[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t v0l = ((uint64_t)blockIdx.x * kSweepWaves + wid) * a.vb;
    const bool live = r < a.R && a.st[r].done == 0u;
    const uint64_t livemask = __ballot(live);
    uint32_t nviol = 0u;
    if (v0l < a.n && livemask != 0ull) {
        const uint32_t v0 = (uint32_t)v0l, v1 = (uint32_t)min((uint64_t)a.n, v0l + a.vb);
        const uint32_t n = a.n;
        const size_t gofs = (size_t)g * n * kLanes;
        const uint8_t* __restrict__ Cb = a.C[t & 1u] + gofs;
        const uint32_t* __restrict__ Cw = reinterpret_cast<const uint32_t*>(Cb);
        uint8_t* __restrict__ Cn = a.C[(t + 1u) & 1u] + gofs;
        uint32_t* __restrict__ tab = a.taboo ? a.taboo + gofs : nullptr;
        // this lane's chain: nCol, epsilon, 1 - (nCol - 1) eps (:402-412, :471-479), its colour set by words
        const uint32_t nl = a.ncolw[r];
        const float el = a.epsr[r], hl = 1.0f - (float)(nl - 1u) * el;
        uint32_t full[MW];
#pragma unroll
        for (int w = 0; w < MW; w++) {
            const uint32_t lo = 32u * (uint32_t)w;
            full[w] = (!live || nl <= lo) ? 0u : nl >= lo + 32u ? ~0u : (1u << (nl - lo)) - 1u;
        }
        uint32_t nmin, nmax;   // the wave's smallest and largest live nCol
        {
            uint32_t lo = live ? nl : 256u, hx = live ? nl : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
                hx = max(hx, (uint32_t)__shfl_xor((int)hx, o, 64));
            }
            nmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            nmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)hx);
        }
        // the wave's table; this lane's column; the columns its four sub-steps OR into
        uint32_t* const occw = s_occ + wid * (uint32_t)(MW * kLanes);
        uint32_t* const mycol = occw + lane;
        uint32_t* const colp[4] = {occw + 4u * i + (q & 3u), occw + 4u * i + ((q + 1u) & 3u),
                                   occw + 4u * i + ((q + 2u) & 3u), occw + 4u * i + ((q + 3u) & 3u)};
        const uint32_t rot = 8u * q;
        // engine state of the block's first vertex: x_r 16807^(t n + v0 + 1)
        uint64_t e = (uint64_t)tn + v0 + 1ull;
        while (e >= kMinstdN) e -= kMinstdN;
        uint32_t pw = 1u;
        for (int k = 0; k < 4; k++) pw = minstd_mulmod(pw, a.powtab[k * 256 + (int)((e >> (8 * k)) & 255u)]);
        uint32_t x = live ? minstd_mulmod(a.xinit[r], pw) : 1u;
        uint32_t grp = 0u, rg = 0u, tstride = 0u;
        if constexpr (TILED) {
            grp = v0 / a.grp_rows;
            rg = v0 - grp * a.grp_rows;
            tstride = tseg_stride(a.grp_rows);
        }
        uint32_t occ[MW];
        auto read_occ = [&]() {
            wave_lds_sync();
#pragma unroll
            for (int w = 0; w < MW; w++)
                occ[w] = __hip_atomic_load(mycol + w * (int)kLanes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        };
        auto all_full = [&]() {
            bool mine = true;
#pragma unroll
            for (int w = 0; w < MW; w++) mine = mine && (occ[w] & full[w]) == full[w];
            return (bool)__all(mine);
        };
        for (uint32_t v = v0; v < v1; v++) {
#pragma unroll
            for (int w = 0; w < MW; w++)
                __hip_atomic_store(mycol + w * (int)kLanes, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            wave_lds_sync();
            uint32_t drained = 0u;
            if constexpr (!TILED) {
                const uint64_t end = min(a.row_off[v + 1], a.m), base = min(a.row_off[v], end);
                const uint64_t deg = end - base;
                uint32_t ids = lane < deg ? a.col_idx[base + lane] : 0u;
                for (uint64_t c0 = 0; c0 < deg; c0 += 64u) {
                    const uint32_t cur = ids;
                    const uint64_t nx = c0 + 64u + lane;
                    ids = nx < deg ? a.col_idx[base + nx] : 0u;   // the next chunk's ids, in flight during this one
                    const uint32_t rem = (uint32_t)min((uint64_t)64u, deg - c0);
                    drain_chunk_wide<MW>(Cw, cur, rem, q, i, n - 1u, rot, colp);
                    drained += rem;
                    if (drained >= nmin) {
                        read_occ();
                        if (all_full()) break;
                    }
                }
            } else {
                const uint16_t* __restrict__ ids16 = a.tcol + a.gbase[grp];
                const uint32_t* __restrict__ ts = a.tseg + (size_t)grp * a.nblocks * tstride + rg;
                bool rowfull = false;
                for (uint32_t b0 = 0; b0 < a.nblocks && !rowfull; b0 += 64u) {
                    // directory of blocks b0 .. b0 + 63, as in chains_sweep_kernel
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
                    if (total == 0u) continue;
                    uint32_t ids = tiled_chunk(ids16, delta, endo, 0u, total, b0, a.block_log2, lane);
                    for (uint32_t c0 = 0; c0 < total; c0 += 64u) {
                        const uint32_t cur = ids;
                        if (c0 + 64u < total)   // the next chunk's ids, in flight during this one
                            ids = tiled_chunk(ids16, delta, endo, c0 + 64u, total, b0, a.block_log2, lane);
                        const uint32_t rem = min(64u, total - c0);
                        drain_chunk_wide<MW>(Cw, cur, rem, q, i, n - 1u, rot, colp);
                        drained += rem;
                        if (drained >= nmin) {
                            read_occ();
                            rowfull = all_full();
                            if (rowfull) break;
                        }
                    }
                }
                if (++rg == a.grp_rows) {
                    rg = 0u;
                    grp++;
                }
            }
            read_occ();
            const uint32_t c = Cb[(size_t)v * kLanes + lane];
            uint32_t ownw = 0u, Zv = 0u;
#pragma unroll
            for (int w = 0; w < MW; w++) {
                if ((c >> 5) == (uint32_t)w) ownw = occ[w];
                Zv += (uint32_t)__popc(occ[w]);
            }
            const bool viol = (ownw >> (c & 31u)) & 1u;
            nviol += (live && viol) ? 1u : 0u;
            if constexpr (FLAGS) {
                const uint64_t fb = __ballot(viol);
                uint64_t* fw = a.vfl + ((size_t)(t & 1u) * a.G + g) * n + v;
                if (lane == 0u) *fw = (*fw & ~livemask) | (fb & livemask);
            }
            uint32_t tb = tab ? tab[(size_t)v * kLanes + lane] : 0u;
            uint32_t newc = c;
            bool ovf = false;
            const bool walk = live && tb == 0u;
            const uint32_t fr = nl - Zv;
            if (__any(walk)) {
                const float u = minstd_canonical(x);
                const bool own = !viol || fr == 0u;
                const float ps = own ? hl : (1.0f - el * (float)Zv) / (float)fr;
                float cdf = 0.0f;
                uint32_t idx = nl;   // "not found" is the chain's own nCol: an overflow exactly when its oracle has one
                bool stop = false;
#pragma unroll
                for (int w = 0; w < MW; w++) {
                    const uint32_t kb = 32u * (uint32_t)w;
                    if (!stop && kb < nmax) {
                        // colours of this word whose p is ps; eps elsewhere
                        const uint32_t Sw = own ? ((c >> 5) == (uint32_t)w ? 1u << (c & 31u) : 0u) : ~occ[w];
                        const uint32_t kend = min(kb + 32u, nmax);
                        for (uint32_t k0 = kb; k0 < kend; k0 += 8u) {
                            const uint32_t k1 = min(k0 + 8u, kend);
                            for (uint32_t k = k0; k < k1; k++) {
                                if (k < nl) {
                                    cdf += ((Sw >> (k & 31u)) & 1u) ? ps : el;
                                    if (idx == nl && cdf > u) idx = k;   // strict >, the first colour only (:510-514)
                                }
                            }
                            if (__all(!walk || idx != nl || k1 >= nl)) {
                                stop = true;
                                break;
                            }
                        }
                    }
                }
                if (walk) {
                    ovf = idx == nl;
                    newc = ovf ? c : idx;
                    tb = (newc == c) ? a.taboo_it : 0u;   // :526 (an overflow's is written by the commit)
                }
            }
            if (live && !walk) tb--;   // :496-501
            if (live) {
                Cn[(size_t)v * kLanes + lane] = (uint8_t)newc;
                if (tab) tab[(size_t)v * kLanes + lane] = tb;
            }
            const uint64_t ob = __ballot(ovf);
            if (ob != 0ull && lane == 0u) {
                const uint32_t slot = atomicAdd(&a.evcnt[(t & 1u) * a.G + g], 1u);
                if (slot < n) a.evlist[(size_t)g * n + slot] = make_uint4(v, (uint32_t)ob, (uint32_t)(ob >> 32), 0u);
            }
            x = minstd_mulmod(x, kMinstdA);
        }
        if (nviol) atomicAdd(&s_viol[lane], nviol);
    }
    __syncthreads();
    if (threadIdx.x < kLanes && s_viol[threadIdx.x]) atomicAdd(&a.viol[g * kLanes + threadIdx.x], s_viol[threadIdx.x]);
}

constexpr uint32_t kHistWideWaves = 4;
constexpr uint32_t kHistWideMaxV = 65504u;   // vertices per workgroup: a 16-bit counter cannot carry; a multiple of 32

// Class sizes of a batch whose largest nCol is above 64: hist[r][k], k < 256, a.hist rows of 256.
// The loads and the per-byte buffer select are chains_hist_kernel's. The LDS table is
// [64 chains][128 words], two 16-bit counters per word (colour k in half k & 1 of word k >> 1, 32 KB):
// a workgroup counts at most kHistWideMaxV < 2^16 vertices, so no counter carries into its
// neighbour and the result is exact. The word is rotated by the chain to spread the banks.
__global__ __launch_bounds__(64 * kHistWideWaves) void chains_hist_wide_kernel(ChainArgs a, uint32_t t, uint32_t hv) {
    __shared__ uint32_t s_h[kLanes * 128u];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u, wid = threadIdx.x >> 6;
    const uint32_t g = blockIdx.y, n = a.n;
    for (uint32_t k = threadIdx.x; k < kLanes * 128u; k += 64u * kHistWideWaves) s_h[k] = 0u;
    __syncthreads();
    uint32_t sel = 0u, valid = 0u, vbytes = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t r = g * kLanes + 4u * i + j;
        if (r < a.R) {
            valid |= 1u << j;
            vbytes |= 255u << (8u * j);
            const uint32_t buf = a.st[r].done ? a.st[r].buf : (t & 1u);
            if (buf & 1u) sel |= 255u << (8u * j);
        }
    }
    const uint32_t need1 = sel, need0 = vbytes & ~sel;
    const size_t gofs = (size_t)g * n * kLanes;
    const uint32_t* __restrict__ W0 = reinterpret_cast<const uint32_t*>(a.C[0] + gofs);
    const uint32_t* __restrict__ W1 = reinterpret_cast<const uint32_t*>(a.C[1] + gofs);
    const uint64_t vb0 = (uint64_t)blockIdx.x * hv;
    const uint32_t vend = (uint32_t)min((uint64_t)n, vb0 + hv);
    for (uint64_t vt = vb0 + 32ull * wid; vt < vend; vt += 32ull * kHistWideWaves) {
        uint32_t w[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const uint64_t v = vt + 4u * k + q;
            uint32_t w0 = 0u, w1 = 0u;
            if (v < vend) {
                if (need0) w0 = W0[(size_t)v * 16u + i];
                if (need1) w1 = W1[(size_t)v * 16u + i];
            }
            w[k] = (w0 & ~sel) | (w1 & sel);
        }
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            if (vt + 4u * k + q < vend) {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) {
                    const uint32_t ch = 4u * i + j, col = (w[k] >> (8u * j)) & 255u;
                    if ((valid >> j) & 1u) atomicAdd(&s_h[ch * 128u + (((col >> 1) + ch) & 127u)], 1u << (16u * (col & 1u)));
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kLanes * 128u; k += 64u * kHistWideWaves) {
        const uint32_t cnt = s_h[k], ch = k >> 7, col = 2u * (((k & 127u) - ch) & 127u);
        uint32_t* row = a.hist + ((size_t)g * kLanes + ch) * 256u;
        if (cnt & 0xFFFFu) atomicAdd(&row[col], cnt & 0xFFFFu);
        if (cnt >> 16) atomicAdd(&row[col + 1u], cnt >> 16);
    }
}
