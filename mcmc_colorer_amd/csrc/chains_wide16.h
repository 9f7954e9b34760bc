// mcmc_colorer_amd/csrc/chains_wide16.h -- the half-word sweep of the batched chains: per-lane nCol up to 2048.
//
// Included by chains.hip inside namespace mcmc::{anonymous}, after chains_wide.h (wave_lds_sync) and
// with cdf_walk.h in scope. A colour is a uint16_t, C16[buffer][group][v][64]: one neighbour's colours
// of a whole group are 128 contiguous bytes. ChainArgs::C keeps its type; the kernels here and the
// element-typed init / commit kernels of chains.hip read it as half-words. The grid, the row sources
// (CSR / flattened tiled layout), the engine stepping, the taboo handling, the overflow records and the
// violator counts are the wide sweep's (chains_wide.h); what follows is what differs.
//
// Drain: the wave-load keeps its lane geometry. Lane (q = l >> 4, i = l & 15) loads the 8-byte word of
//   chains 4 i .. 4 i + 3 of neighbour q of the step's four: 512 B per wave-load, eight in flight before
//   the first use (16 VGPRs). The word is rotated right by 16 q once, so that half-word j of it is
//   chain 4 i + ((j + q) & 3): in each of a step's four LDS instructions the 64 lanes address 64
//   distinct columns, as in chains_wide.h -- no per-quarter copies of the table, no cross-quarter
//   reduction.
// Table: each wave owns occ[MW][64] 32-bit words (column l = chain l, row w = colours 32 w .. 32 w + 31)
//   and cnt[64], MW = 16, 32 or 64 for a largest nCol <= 512, <= 1024, <= 2048: 4.25, 8.25 or 16.25 KB
//   per wave. Workgroups are 4 waves at MW = 16 and 32 (17.25 and 33.25 KB of static LDS) and 2 waves at
//   MW = 64 (32.75 KB): every instantiation stays under the 64 KB of a static block and four
//   workgroups of the larger two fit a CU's 160 KB. Only the words a live chain can use (the wave's
//   largest live nCol) are cleared per vertex.
// Counted OR: MW words per lane do not fit in registers, so nothing of the table is kept there. A
//   sub-step is a RETURNING ds_or_b32 of 1 << (c & 31) at row c >> 5; where the returned word did not
//   hold the bit yet, the lane adds 1 to cnt[that chain] (ds_add_u32, the same 64 distinct columns). A
//   chain's counter is therefore its Zv at any time: no popcount pass, and the row's exit test is one
//   LDS read per lane per chunk (cnt == nCol_l for every live lane; skipped while fewer neighbours are
//   drained than the wave's smallest live nCol). Slots past the row's end re-read the chunk's first
//   neighbour: the bit is set by then, so nothing is counted twice. The own-colour test is one read
//   of word c >> 5.
// Walk: no step-by-step walk over up to 2048 colours. A lane that draws calls cdf_walk.h with its own
//   (nCol, eps, u): walk_own(nCol, c, eps, hi, u) where the chain keeps its colour's weight (no
//   violation, or no free colour), else walk_mask over its LDS column through OccCol (a strided view:
//   element w is word w of the column) with pf = (1 - eps Zv) / fr. Both are exact fp32 over runs and
//   binades and return nCol for "not found", the overflow's mark. Lanes diverge here by design.
// Class sizes (chains_hist16_kernel): the chain-subset design of chains_hist_wide_kernel, not global
//   atomics -- a uniform batch of few colours would send n x R atomics to a handful of L2 lines. A
//   workgroup counts 16384 / hc chains (hc = 32 MW columns: 32, 16 or 8 chains) of a vertex chunk in a
//   32 KB table of packed 16-bit counters, at most 65504 vertices so that no counter carries, then
//   adds its nonzero cells to the global rows of hc words.
// FLAGS (mcmc_chains_enable_repair16, chains_tailcut16.h): as in chains_sweep_kernel, lane 0 keeps the
//   ballot of `viol` per (group, v) in a.vfl[t & 1], merged under the live mask. The FLAGS = false code
//   objects are the ones below, unchanged.
//
// Resources (hipcc -O3 -ffp-contract=off, gfx950, -Rpass-analysis=kernel-resource-usage):
//   chains_sweep_wide16_kernel  <CSR, 16>    <CSR, 32>    <CSR, 64>    <tiled, 16>  <tiled, 32>  <tiled, 64>
//   VGPRs                       68           74           74           81           81           81
//   SGPRs                       99           99           99           106          106          106
//   scratch (bytes / lane)      0            0            0            0            0            0
//   LDS (bytes)                 17664        34048        33536        17664        34048        33536
//   FLAGS = true: the same VGPRs, scratch and LDS; SGPRs 105 (CSR) and 106 (tiled).
#pragma once

// a wave-private LDS column seen as the `mask` of cdf_walk.h's walk_mask: element w is word w
struct OccCol {
    uint32_t w[kLanes];
    __device__ __forceinline__ operator uint32_t() const { return w[0]; }
};

constexpr int wide16_waves(int MW) { return MW == 64 ? 2 : 4; }

// K steps of the drain from step s0 of the chunk whose ids `cur` holds: K 8-byte loads issued, then
// K x 4 counted ORs. colp[j] / cntp[j]: word 0 of the column, and the counter, of chain
// 4 i + ((j + q) & 3); rot = 16 q.
template <int K, int MW>
__device__ __forceinline__ void drain_steps_wide16(const uint64_t* __restrict__ Cq, uint32_t cur, uint32_t s0, uint32_t rem,
                                                   uint32_t q, uint32_t i, uint32_t nlast, uint32_t rot,
                                                   uint32_t* const (&colp)[4], uint32_t* const (&cntp)[4]) {
    uint64_t w[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nlast);
        w[k] = Cq[(size_t)id * 16u + i];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint64_t wr = (w[k] >> rot) | (w[k] << ((64u - rot) & 63u));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c = (uint32_t)(wr >> (16 * j)) & 0xFFFFu;
            const uint32_t bit = 1u << (c & 31u);
            // rows past MW - 1 folded back: a colour is below its chain's nCol <= 32 MW
            const uint32_t old = __hip_atomic_fetch_or(colp[j] + ((c >> 5) & (uint32_t)(MW - 1)) * kLanes, bit,
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (!(old & bit)) (void)__hip_atomic_fetch_add(cntp[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
}

// the 4-neighbour steps over the `rem` ids of `cur`
template <int MW>
__device__ __forceinline__ void drain_chunk_wide16(const uint64_t* __restrict__ Cq, uint32_t cur, uint32_t rem, uint32_t q,
                                                   uint32_t i, uint32_t nlast, uint32_t rot, uint32_t* const (&colp)[4],
                                                   uint32_t* const (&cntp)[4]) {
    for (uint32_t s = 0; 4u * s < rem;) {
        if (rem - 4u * s > 16u) {
            drain_steps_wide16<8, MW>(Cq, cur, s, rem, q, i, nlast, rot, colp, cntp);
            s += 8u;
        } else {
            drain_steps_wide16<4, MW>(Cq, cur, s, rem, q, i, nlast, rot, colp, cntp);
            s += 4u;
        }
    }
}

// TILED as in chains_sweep_kernel. MW: 32-bit words of a chain's occupancy column (16: every nCol <= 512,
// 32: <= 1024, 64: <= 2048). nCol, epsilon, hi, fr, pf and the walk's end are per lane (a.ncolw, a.epsr).
// FLAGS as in chains_sweep_kernel.
template <bool TILED, int MW, bool FLAGS>
__global__ __launch_bounds__(64 * wide16_waves(MW)) void chains_sweep_wide16_kernel(ChainArgs a, uint32_t t, uint32_t tn) {
    constexpr uint32_t kWaves = (uint32_t)wide16_waves(MW);
    if (*a.ndone >= a.R) return;   // every chain stopped (workgroup-uniform)
    __shared__ uint32_t s_viol[kLanes];
    __shared__ uint32_t s_occ[kWaves * MW * kLanes];
    __shared__ uint32_t s_cnt[kWaves * kLanes];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.y, r = g * kLanes + lane;
    if (threadIdx.x < kLanes) s_viol[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t v0l = ((uint64_t)blockIdx.x * kWaves + wid) * a.vb;
    const bool live = r < a.R && a.st[r].done == 0u;
    const uint64_t livemask = __ballot(live);
    uint32_t nviol = 0u;
    if (v0l < a.n && livemask != 0ull) {
        const uint32_t v0 = (uint32_t)v0l, v1 = (uint32_t)min((uint64_t)a.n, v0l + a.vb);
        const uint32_t n = a.n;
        const size_t gofs = (size_t)g * n * kLanes;   // in elements: half-words here
        const uint16_t* __restrict__ Ch = reinterpret_cast<const uint16_t*>(a.C[t & 1u]) + gofs;
        const uint64_t* __restrict__ Cq = reinterpret_cast<const uint64_t*>(Ch);
        uint16_t* __restrict__ Cn = reinterpret_cast<uint16_t*>(a.C[(t + 1u) & 1u]) + gofs;
        uint32_t* __restrict__ tab = a.taboo ? a.taboo + gofs : nullptr;
        // this lane's chain: nCol, epsilon, 1 - (nCol - 1) eps (:402-412, :471-479)
        const uint32_t nl = a.ncolw[r];
        const float el = a.epsr[r], hl = 1.0f - (float)(nl - 1u) * el;
        uint32_t nmin, nw;   // the wave's smallest live nCol; the words its largest live nCol uses
        {
            uint32_t lo = live ? nl : 2048u, hx = live ? nl : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
                hx = max(hx, (uint32_t)__shfl_xor((int)hx, o, 64));
            }
            nmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            nw = min(((uint32_t)__builtin_amdgcn_readfirstlane((int)hx) + 31u) >> 5, (uint32_t)MW);
        }
        // the wave's table and counters; this lane's column; the columns its four sub-steps OR into
        uint32_t* const occw = s_occ + wid * (uint32_t)(MW * kLanes);
        uint32_t* const cntw = s_cnt + wid * kLanes;
        uint32_t* const mycol = occw + lane;
        const uint32_t ch4[4] = {4u * i + (q & 3u), 4u * i + ((q + 1u) & 3u), 4u * i + ((q + 2u) & 3u),
                                 4u * i + ((q + 3u) & 3u)};
        uint32_t* const colp[4] = {occw + ch4[0], occw + ch4[1], occw + ch4[2], occw + ch4[3]};
        uint32_t* const cntp[4] = {cntw + ch4[0], cntw + ch4[1], cntw + ch4[2], cntw + ch4[3]};
        const uint32_t rot = 16u * q;
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
        // every live chain's counter has reached its nCol: the rest of the row cannot change anything
        auto all_full = [&]() {
            wave_lds_sync();
            const uint32_t z = __hip_atomic_load(cntw + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            return (bool)__all(!live || z == nl);
        };
        for (uint32_t v = v0; v < v1; v++) {
            for (uint32_t w = 0; w < nw; w++)
                __hip_atomic_store(mycol + w * kLanes, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __hip_atomic_store(cntw + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
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
                    drain_chunk_wide16<MW>(Cq, cur, rem, q, i, n - 1u, rot, colp, cntp);
                    drained += rem;
                    if (drained >= nmin && all_full()) break;
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
                        drain_chunk_wide16<MW>(Cq, cur, rem, q, i, n - 1u, rot, colp, cntp);
                        drained += rem;
                        if (drained >= nmin) {
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
            wave_lds_sync();
            const uint32_t c = Ch[(size_t)v * kLanes + lane];
            const uint32_t Zv = __hip_atomic_load(cntw + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            const uint32_t ownw = __hip_atomic_load(mycol + ((c >> 5) & (uint32_t)(MW - 1)) * kLanes, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_WAVEFRONT);
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
            if (walk) {   // lanes diverge: each walks its own runs and binades
                const float u = minstd_canonical(x);
                const uint32_t fr = nl - Zv;
                uint32_t idx;   // "not found" is the chain's own nCol: an overflow exactly when its oracle has one
                if (!viol || fr == 0u) {
                    idx = walk_own(nl, c, el, hl, u);
                } else {
                    const float pf = (1.0f - el * (float)Zv) / (float)fr;
                    idx = walk_mask(reinterpret_cast<const OccCol*>(mycol), nl, el, pf, u);
                }
                ovf = idx == nl;
                newc = ovf ? c : idx;
                tb = (newc == c) ? a.taboo_it : 0u;   // :526 (an overflow's is written by the commit)
            }
            if (live && !walk) tb--;   // :496-501
            if (live) {
                Cn[(size_t)v * kLanes + lane] = (uint16_t)newc;
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

constexpr uint32_t kHist16Threads = 256;
constexpr uint32_t kHist16Words = 8192;   // the LDS table: 16384 packed 16-bit counters

// Class sizes of a half-word batch: hist[r][k], k < hc = 1 << hc_log2 (512, 1024 or 2048), a.hist rows
// of hc. Grid (vertex chunks of hv <= kHistWideMaxV, group x chain subsets): a workgroup counts
// cs = 16384 / hc chains; thread j is chain j % cs of the subset and takes every (256 / cs)-th vertex
// of the chunk, from the buffer its chain stopped in. Colour k of chain ch counts in half k & 1 of word
// ch hc / 2 + k / 2: at most hv < 2^16 per counter, so none carries and the result is exact.
__global__ __launch_bounds__(kHist16Threads) void chains_hist16_kernel(ChainArgs a, uint32_t t, uint32_t hv, uint32_t hc_log2) {
    __shared__ uint32_t s_h[kHist16Words];
    const uint32_t cs_log2 = 14u - hc_log2, cs = 1u << cs_log2, subs = kLanes >> cs_log2;
    const uint32_t g = blockIdx.y / subs, c0 = (blockIdx.y % subs) << cs_log2, n = a.n;
    for (uint32_t k = threadIdx.x; k < kHist16Words; k += kHist16Threads) s_h[k] = 0u;
    __syncthreads();
    const uint32_t ch = threadIdx.x & (cs - 1u), r = g * kLanes + c0 + ch;
    const uint64_t vb0 = (uint64_t)blockIdx.x * hv;
    const uint32_t vend = (uint32_t)min((uint64_t)n, vb0 + hv);
    if (r < a.R) {
        const uint32_t buf = a.st[r].done ? a.st[r].buf : (t & 1u);
        const uint16_t* __restrict__ Cc = reinterpret_cast<const uint16_t*>(a.C[buf & 1u]) + (size_t)g * n * kLanes + c0 + ch;
        for (uint64_t v = vb0 + (threadIdx.x >> cs_log2); v < vend; v += kHist16Threads >> cs_log2) {
            const uint32_t col = Cc[(size_t)v * kLanes] & ((1u << hc_log2) - 1u);
            atomicAdd(&s_h[(ch << (hc_log2 - 1u)) + (col >> 1)], 1u << (16u * (col & 1u)));
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kHist16Words; k += kHist16Threads) {
        const uint32_t cnt = s_h[k];
        if (cnt == 0u) continue;
        const uint32_t col = 2u * (k & ((1u << (hc_log2 - 1u)) - 1u));
        uint32_t* row = a.hist + (((size_t)g * kLanes + c0 + (k >> (hc_log2 - 1u))) << hc_log2);
        if (cnt & 0xFFFFu) atomicAdd(&row[col], cnt & 0xFFFFu);
        if (cnt >> 16) atomicAdd(&row[col + 1u], cnt >> 16);
    }
}
