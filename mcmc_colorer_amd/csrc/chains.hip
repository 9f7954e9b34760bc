// mcmc_colorer_amd/csrc/chains.hip -- batched independent MCMC chains: one wave lane per chain.
//
// R chains of one graph run as one batch (mcmc_chains_*, include/mcmc_hip.h). Chain r is, bit for
// bit, ColoringMCMC_CPU(g, params, seed + r).run() (graph_coloring/coloringMCMC_CPU.cpp:115-270) with
// its OWN glibc rand() stream for the CDF-overflow fallback (:518) -- unlike --repet, whose
// repetition i + 1 continues the process stream where repetition i stopped.
//
// Layout: colours are bytes, chain-minor in groups of 64 chains, C[buffer][group][v][64], double
// buffered (C_t in buffer t & 1). One neighbour's colours of a whole group are 64 contiguous bytes,
// and lane l of a wave is chain 64 group + l.
//
// Sweep (chains_sweep_kernel): a wave owns `vb` consecutive vertices of one group (blockIdx.y).
//   drain   The row's neighbour ids are wave-uniform: 64 of them per coalesced load (CSR) or per
//           flattened chunk of the tiled 16-bit layout (below), the next 64 prefetched meanwhile. A
//           step loads four neighbours with one instruction: lane l the
//           dword of chains 4 (l & 15) .. +3 of neighbour l >> 4 (256 B per wave-load; the id comes
//           from the id register by ds_bpermute), eight steps in flight before the first use. Every
//           lane ORs the bytes into four partial 64-bit occupancy masks. After 64 neighbours the
//           masks are OR-reduced across the four 16-lane quarters (ds_bpermute xor 16 / 32, no LDS
//           memory); when every live chain's mask holds all nCol colours the row's scan stops
//           (count_free_colors, :361-383, cannot change any more: the result is the same). Slots past
//           the row's end re-read the chunk's first neighbour (OR is idempotent): no predication.
//   tiled   A generated graph (mcmc_graph_er_fast) has no CSR: its rows live in the tiled layout
//           (TiledLayout, mcmc_common.h) as nblocks separate segments of block-local 16-bit ids,
//           each padded to whole octets (8 ids) with copies of its first id. The second
//           instantiation of the sweep flattens a row instead of walking segments (~6 ids each at
//           n = 1e6, degree 100; many empty). Directory: per round of 64 blocks lane j reads the two
//           table entries of block 64 round + j and keeps the segment's start and its count of
//           real ids (padded length less the padding count in the entry's low 3 bits); a wave
//           inclusive scan (__shfl_up) gives every segment its first and end slot in the round's
//           stream of real ids. Chunk: lane j owns slot c0 + j; the owning segment is the number of
//           segments that end at or before the slot (ends ascend, empty segments drop out), found
//           by a binary search over the lanes' ends (six ds_bpermute); one more fetches the
//           segment's start - first slot, the lane loads its 16-bit id and forms
//           (block << block_log2) | id. From the id register on the drain is the CSR one, with the
//           CSR's slot count; the exit test runs after every chunk, ahead of the next directory round.
//   update  Lane l then takes chain l's mask (from lane l >> 2, word l & 3) and runs fill_p
//           ("Baseline", :392-481) + extract_new_color (:492-528) for its chain: own colour,
//           violation bit, Zv = popcount, the sequential fp32 CDF walk with strict `cdf > u`, the
//           taboo counter. u is generate_canonical of engine draw initDraws_r + t n + v + 1: the
//           state is x_r 16807^(t n + v0 + 1) at the block's first vertex (one table powmod, four
//           mulmods) and one mulmod per vertex after it.
//   out     C* bytes; the chain's violator count of C_t (per-lane sum over the block, LDS sum over
//           the workgroup's waves, one atomic per workgroup and chain); one record {v, lane mask}
//           per (group, vertex) with a CDF overflow in the group's append-only list -- at most n
//           records per group, so the list cannot overflow.
// Commit (chains_commit_kernel): one wave per chain. Appends the count to the chain's trajectory,
//   applies `iter > maxRip` and `Cviol <= z` (a chain that stops keeps C_t: the sweep's output for
//   it is discarded, no glibc draw is taken, and its lanes never write a buffer again), else serves
//   the chain's overflow records in ascending vertex order (wave min-scan of the group's list per
//   event -- events are ~1e-7 per draw) from the chain's glibc window: colour rand() % (nCol - 1)
//   and the taboo value (:518-526). The last chain to stop makes later launches return at once.
// Init (chains_init_kernel): one lane per chain walks default_random_engine(seed_r) through
//   uniform_int_distribution(0, nCol_r - 1) in vertex order, rejections included (:53-61), so
//   initDraws differs per chain and is exact without a host replay. seed_r and the distribution's
//   constants come from a per-chain table the host builds.
// Ladder (mcmc_chains_create_ladder): chain r has its own nCol_r, eps_r and seed_r. The sweep's
//   LADDER instantiations (CSR and tiled) read nCol and epsilon per lane; the uniform instantiations
//   are the code objects they were (63 / 70 and 67 / 91 VGPRs / SGPRs, no scratch). A lane's four
//   partial masks belong to four chains of four widths: their nCol travel as four bytes of one
//   VGPR, every mask starts at the complement of its chain's colour set (all ones when the chain is
//   not live), and "every live mask full" is "all four all ones" whatever the widths. The update
//   takes mask & full_lane; hi, fr, ps and the walk's "not found" value are the lane's own; the walk
//   runs to the wave's largest live nCol (one wave reduction per block), a lane adding and testing
//   only while k < nCol_l, in the same fp32 order as the single run. The commit draws
//   rand() % (nCol_r - 1).
// Wide (mcmc_chains_create_wide, chains_wide.h): per-chain nCol up to 256. chains_sweep_wide_kernel<TILED, MW>
//   keeps the layout, the grid, the drain's wave-load, the row sources and everything from the update's
//   taboo on; a chain's occupancy is MW = 4 or 8 words of a wave-private LDS table, set by ds_or_b32 with
//   64 distinct columns per instruction, and read back by the chain's lane. The sweeps above are
//   untouched: they read the byte table a.ncol, the wide sweep and the commit the 16-bit a.ncolw.
//   Batches above 64 colours count their class sizes with chains_hist_wide_kernel (rows of 256).
// Wide16 (mcmc_chains_create_wide16, chains_wide16.h): per-chain nCol up to 2048, colours as uint16_t
//   (C16[buffer][group][v][64]). chains_sweep_wide16_kernel<TILED, MW> has MW = 16, 32 or 64 table words per
//   chain, counts newly set bits with the returning ds_or so that a chain's Zv is one LDS word, and walks
//   the CDF with cdf_walk.h per lane. The init and commit kernels are templates over the colour element;
//   class sizes come from chains_hist16_kernel; its tail cut is mcmc_chains_enable_repair16 (chains_tailcut16.h:
//   half-word normalise, recount and repair kernels, the colour order in global memory, walked by a whole wave).
// Tail cut (mcmc_chains_enable_repair, chains_tailcut.h): after the loop every chain that stopped with
//   violators is repaired as the single run's corrected tail cut repairs it, 64 chains per row read; the
//   sweeps' FLAGS instantiations keep the violator ballots its first pass needs.
// Histograms (chains_hist_kernel): hist[r][k] = vertices of colour k in chain r's final colouring,
//   read from the buffer each chain stopped in (selected per byte of the drain's dword), counted in
//   an LDS table [64 chains][64 colours], one global atomic per nonzero cell and workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cdf_walk.h"
#include "mcmc_common.h"
#include "rng.h"

namespace mcmc {
namespace {

constexpr uint32_t kLanes = 64;              // chains per group = lanes per wave
constexpr uint32_t kMaxChains = 1024;
constexpr uint32_t kSweepWaves = 4;          // waves per sweep workgroup
constexpr uint32_t kTrajCapMax = 1u << 20;   // trajectory entries kept per chain, as mcmc_run
constexpr uint32_t kPollSweeps = 8;          // sweeps between two reads of the all-done counter

struct ChainState {      // per chain, device
    uint32_t done, iter, maxIter, buf;
    uint32_t finalViol, head, draws_lo, draws_hi;   // head: the glibc ring's oldest word
};

struct ChainArgs {
    const uint64_t* row_off;
    const uint32_t* col_idx;
    uint64_t m;
    // the full-range tiled layout of a generated graph (row_off == nullptr): chains_sweep_kernel<true>
    const uint16_t* tcol;
    const uint64_t* gbase;
    const uint32_t* tseg;
    uint32_t grp_rows, nblocks, block_log2;
    uint32_t n, R, G, nCol, vb;
    uint32_t taboo_it, z, maxRip, traj_cap;
    float eps;
    uint8_t* C[2];          // [G][n][64] bytes; uint16_t elements in a half-word batch (chains_wide16.h)
    uint32_t* taboo;        // [G][n][64], nullptr when tabooIteration == 0
    uint32_t* xinit;        // [G * 64] engine state after the initial colouring
    uint64_t* init_draws;   // [G * 64]
    const uint32_t* powtab; // [4][256]: 16807^(b 256^k)
    uint32_t* viol;         // [G * 64] violators of C_t, zeroed by the commit
    uint32_t* evcnt;        // [2][G] overflow records of sweep t in evcnt[t & 1]
    uint4* evlist;          // [G][n] {v, lanes 0..31, lanes 32..63, 0}
    ChainState* st;         // [G * 64]
    uint32_t* ring;         // [G * 64][31] glibc windows as rings
    uint32_t* traj;         // [R][traj_cap]
    uint32_t* ndone;        // chains that stopped
    // per chain (a ladder's differ; a uniform batch holds nCol, eps in every entry): the ladder
    // instantiations of the sweep, the commit's rand() % (nCol_r - 1)
    const uint8_t* ncol;    // [G * 64], 0 past R (the narrow ladder sweeps; a wide batch's entries are not read)
    const float* epsr;      // [G * 64]
    uint32_t* hist;         // [G * 64][64 or 256] class sizes of the final colourings (chains_hist_kernel / _wide_); rows of 512, 1024 or 2048 in a half-word batch
    const uint16_t* ncolw;  // [G * 64], 0 past R: nCol up to 2048 (the wide and half-word sweeps, the commit)
    uint64_t* vfl;          // [2][G][n] violator ballots of sweep t in vfl[t & 1] (the FLAGS sweeps; chains_tailcut.h)
};

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t or_xor64(uint64_t x, int lane_mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, lane_mask, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), lane_mask, 64);
    return x | (((uint64_t)hi << 32) | lo);
}

// K steps of the drain from step s0 of the chunk whose ids `cur` holds (lane j: neighbour j of the
// chunk, `rem` of them valid): K loads issued, then K x 4 bytes ORed into the partial masks.
template <int K>
__device__ __forceinline__ void drain_steps(const uint32_t* __restrict__ Cw, uint32_t cur, uint32_t s0, uint32_t rem,
                                            uint32_t q, uint32_t i, uint32_t nmax, uint64_t (&m)[4]) {
    uint32_t w[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (s0 + (uint32_t)k) * 4u + q;
        const uint32_t id = min((uint32_t)__shfl((int)cur, (int)(e < rem ? e : 0u), 64), nmax);
        w[k] = Cw[(size_t)id * 16u + i];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] |= 1ull << ((w[k] >> (8 * j)) & 63u);
    }
}

// One chunk of the drain, shared by the CSR and the tiled instantiation: the 4-neighbour steps over
// the `rem` ids of `cur`, the OR-reduction of the partial masks over the four quarters, and the exit
// test -- `all_full`: every live chain's mask is full. A macro, not a function: through a function
// (forced inline) the CSR sweep compiled to 81 VGPRs instead of 63. Ladder: a mask starts at the
// complement of its chain's own colour set (all ones for a chain that is not live), so "full" is all
// ones for every width; the test is skipped while fewer neighbours are drained than the smallest
// live nCol of the wave (it cannot succeed).
#define MCMC_DRAIN_CHUNK(cur, rem, all_full)                                                        \
    do {                                                                                            \
        for (uint32_t s = 0; 4u * s < (rem);) {                                                     \
            if ((rem) - 4u * s > 16u) {                                                             \
                drain_steps<8>(Cw, (cur), s, (rem), q, i, n - 1u, m);                               \
                s += 8u;                                                                            \
            } else {                                                                                \
                drain_steps<4>(Cw, (cur), s, (rem), q, i, n - 1u, m);                               \
                s += 4u;                                                                            \
            }                                                                                       \
        }                                                                                           \
        _Pragma("unroll") for (int j = 0; j < 4; j++) m[j] = or_xor64(or_xor64(m[j], 16), 32);      \
        if constexpr (LADDER) {                                                                     \
            drained += (rem);                                                                       \
            all_full = drained >= nmin && __all((m[0] & m[1] & m[2] & m[3]) == ~0ull);              \
        } else {                                                                                    \
            bool mine = true;                                                                       \
            _Pragma("unroll") for (int j = 0; j < 4; j++)                                           \
                mine = mine && (m[j] == full || ((dead4 >> j) & 1u));                               \
            all_full = __all(mine);                                                                 \
        }                                                                                           \
    } while (0)

// Tiled layout: the ids of slots c0 .. c0 + 63 of a directory round's flattened stream (lane j: slot
// c0 + j). endo: the end slot of lane j's segment in the stream (ascending over the lanes); delta:
// its start in the group's ids minus its first slot; b0: the round's first block. The owner of a
// slot is the number of segments that end at or before it: a binary search over the lanes' endo, six
// ds_bpermute. Slots past `total` read the group's first id (in bounds; the drain never uses them).
__device__ __forceinline__ uint32_t tiled_chunk(const uint16_t* __restrict__ ids16, uint32_t delta, uint32_t endo,
                                                uint32_t c0, uint32_t total, uint32_t b0, uint32_t block_log2,
                                                uint32_t lane) {
    const uint32_t p = c0 + lane;
    uint32_t sg = 0u;
#pragma unroll
    for (uint32_t step = 32u; step > 0u; step >>= 1)
        if ((uint32_t)__shfl((int)endo, (int)(sg + step - 1u), 64) <= p) sg += step;   // sg <= 63
    const uint32_t d = (uint32_t)__shfl((int)delta, (int)sg, 64);
    const bool in = p < total;
    return (in ? (b0 + sg) << block_log2 : 0u) | ids16[in ? p + d : 0u];
}

// TILED = false: the rows come from the CSR; true: from the full-range tiled layout.
// LADDER = false: one nCol and epsilon for the batch (kernel arguments, wave-uniform); true: chain r
// has its own nCol_r, eps_r (a.ncol, a.epsr). What differs: the masks' start values and the exit test
// (MCMC_DRAIN_CHUNK), and in the update full, hi, fr, ps and the walk's end are per lane; the walk
// runs to the wave's largest live nCol, a lane adding and testing only while k < nCol_l.
// FLAGS = true (mcmc_chains_enable_repair): lane 0 also keeps the ballot of `viol` per (group, v) in
// a.vfl[t & 1], merged under the live mask so that a stopped chain keeps its bits. One wave owns a
// (group, v): no atomic.
template <bool TILED, bool LADDER, bool FLAGS>
__global__ __launch_bounds__(64 * kSweepWaves) void chains_sweep_kernel(ChainArgs a, uint32_t t, uint32_t tn) {
    if (*a.ndone >= a.R) return;   // every chain stopped (workgroup-uniform)
    __shared__ uint32_t s_viol[kLanes];
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
        const uint32_t n = a.n, nCol = a.nCol;
        const size_t gofs = (size_t)g * n * kLanes;
        const uint8_t* __restrict__ Cb = a.C[t & 1u] + gofs;
        const uint32_t* __restrict__ Cw = reinterpret_cast<const uint32_t*>(Cb);
        uint8_t* __restrict__ Cn = a.C[(t + 1u) & 1u] + gofs;
        uint32_t* __restrict__ tab = a.taboo ? a.taboo + gofs : nullptr;
        const uint64_t full = nCol == 64u ? ~0ull : (1ull << nCol) - 1ull;
        // the four chains this lane's partial masks belong to that are not live count as full
        const uint32_t dead4 = ~(uint32_t)(livemask >> (4u * i)) & 15u;
        const float eps = a.eps, hi = 1.0f - (float)(nCol - 1u) * eps;   // :402-412, :471-479
        // ladder: this lane's chain (nl, el, hl, fulll), the four chains of its partial masks (nc4: their
        // nCol as bytes, 0 where not live), the wave's smallest and largest live nCol
        uint32_t nl = 0u, nc4 = 0u, nmin = 0u, nmax = 0u;
        float el = 0.0f, hl = 0.0f;
        uint64_t fulll = 0ull;
        if constexpr (LADDER) {
            nl = a.ncol[r];
            el = a.epsr[r];
            hl = 1.0f - (float)(nl - 1u) * el;
            fulll = nl == 64u ? ~0ull : (1ull << nl) - 1ull;
            nc4 = reinterpret_cast<const uint32_t*>(a.ncol)[g * 16u + i];
#pragma unroll
            for (int j = 0; j < 4; j++)
                if ((dead4 >> j) & 1u) nc4 &= ~(255u << (8 * j));
            uint32_t lo = live ? nl : 64u, hx = live ? nl : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
                hx = max(hx, (uint32_t)__shfl_xor((int)hx, o, 64));
            }
            nmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            nmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)hx);
        }
        // engine state of the block's first vertex: x_r 16807^(t n + v0 + 1)
        uint64_t e = (uint64_t)tn + v0 + 1ull;
        while (e >= kMinstdN) e -= kMinstdN;
        uint32_t pw = 1u;
        for (int k = 0; k < 4; k++) pw = minstd_mulmod(pw, a.powtab[k * 256 + (int)((e >> (8 * k)) & 255u)]);
        uint32_t x = live ? minstd_mulmod(a.xinit[r], pw) : 1u;
        // tiled: the layout group of v and v's row in it (a wave's rows may straddle two groups)
        uint32_t grp = 0u, rg = 0u, tstride = 0u;
        if constexpr (TILED) {
            grp = v0 / a.grp_rows;
            rg = v0 - grp * a.grp_rows;
            tstride = tseg_stride(a.grp_rows);
        }
        for (uint32_t v = v0; v < v1; v++) {
            uint64_t m[4] = {0ull, 0ull, 0ull, 0ull};
            uint32_t drained = 0u;
            if constexpr (LADDER) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t b = (nc4 >> (8 * j)) & 255u;
                    m[j] = b >= 64u ? 0ull : ~0ull << b;
                }
            }
            if constexpr (!TILED) {
                const uint64_t end = min(a.row_off[v + 1], a.m), base = min(a.row_off[v], end);
                const uint64_t deg = end - base;
                uint32_t ids = lane < deg ? a.col_idx[base + lane] : 0u;
                for (uint64_t c0 = 0; c0 < deg; c0 += 64u) {
                    const uint32_t cur = ids;
                    const uint64_t nx = c0 + 64u + lane;
                    ids = nx < deg ? a.col_idx[base + nx] : 0u;   // the next chunk's ids, in flight during this one
                    const uint32_t rem = (uint32_t)min((uint64_t)64u, deg - c0);
                    bool all_full;
                    MCMC_DRAIN_CHUNK(cur, rem, all_full);
                    if (all_full) break;
                }
            } else {
                const uint16_t* __restrict__ ids16 = a.tcol + a.gbase[grp];
                const uint32_t* __restrict__ ts = a.tseg + (size_t)grp * a.nblocks * tstride + rg;
                bool rowfull = false;
                for (uint32_t b0 = 0; b0 < a.nblocks && !rowfull; b0 += 64u) {
                    // directory of blocks b0 .. b0 + 63: lane j its segment's start and its real ids
                    // (the padded length less the padding count in the entry's low 3 bits)
                    uint32_t seg0 = 0u, len = 0u;
                    if (b0 + lane < a.nblocks) {
                        const uint32_t* ent = ts + (size_t)(b0 + lane) * tstride;
                        const uint32_t e0 = ent[0];
                        seg0 = e0 & kTsegPos;
                        len = (ent[1] & kTsegPos) - seg0 - (e0 & 7u);
                    }
                    uint32_t endo = len;   // inclusive scan: the segment's end slot in the round's stream
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
                        MCMC_DRAIN_CHUNK(cur, rem, rowfull);
                        if (rowfull) break;
                    }
                }
                if (++rg == a.grp_rows) {
                    rg = 0u;
                    grp++;
                }
            }
            // chain `lane`: word lane & 3 of lane lane >> 2
            const int src = (int)(lane >> 2);
            const uint64_t t0 = shfl64(m[0], src), t1 = shfl64(m[1], src), t2 = shfl64(m[2], src), t3 = shfl64(m[3], src);
            const uint32_t jj = lane & 3u;
            const uint64_t mask = (jj == 0u ? t0 : jj == 1u ? t1 : jj == 2u ? t2 : t3) & (LADDER ? fulll : full);
            const uint32_t c = Cb[(size_t)v * kLanes + lane];
            const bool viol = (mask >> c) & 1ull;
            nviol += (live && viol) ? 1u : 0u;
            if constexpr (FLAGS) {
                const uint64_t fb = __ballot(viol);
                uint64_t* fw = a.vfl + ((size_t)(t & 1u) * a.G + g) * n + v;
                if (lane == 0u) *fw = (*fw & ~livemask) | (fb & livemask);
            }
            const uint32_t Zv = (uint32_t)__popcll(mask);
            uint32_t tb = tab ? tab[(size_t)v * kLanes + lane] : 0u;
            uint32_t newc = c;
            bool ovf = false;
            const bool walk = live && tb == 0u;
            if constexpr (!LADDER) {
                const uint32_t fr = nCol - Zv;
                if (__any(walk)) {
                    const float u = minstd_canonical(x);
                    const bool own = !viol || fr == 0u;
                    const uint64_t S = own ? (1ull << c) : ~mask;   // colours whose p is ps; eps elsewhere
                    const float ps = own ? hi : (1.0f - eps * (float)Zv) / (float)fr;
                    float cdf = 0.0f;
                    uint32_t idx = nCol;
                    for (uint32_t k0 = 0; k0 < nCol; k0 += 8u) {
                        const uint32_t k1 = min(k0 + 8u, nCol);
                        for (uint32_t k = k0; k < k1; k++) {
                            cdf += ((S >> k) & 1ull) ? ps : eps;
                            if (idx == nCol && cdf > u) idx = k;   // strict >, the first colour only (:510-514)
                        }
                        if (__all(!walk || idx != nCol)) break;
                    }
                    if (walk) {
                        ovf = idx == nCol;
                        newc = ovf ? c : idx;
                        tb = (newc == c) ? a.taboo_it : 0u;   // :526 (an overflow's is written by the commit)
                    }
                }
            } else {
                const uint32_t fr = nl - Zv;
                if (__any(walk)) {
                    const float u = minstd_canonical(x);
                    const bool own = !viol || fr == 0u;
                    const uint64_t S = own ? (1ull << c) : ~mask;
                    const float ps = own ? hl : (1.0f - el * (float)Zv) / (float)fr;
                    float cdf = 0.0f;
                    uint32_t idx = nl;   // "not found" is the chain's own nCol: an overflow exactly when its oracle has one
                    for (uint32_t k0 = 0; k0 < nmax; k0 += 8u) {
                        const uint32_t k1 = min(k0 + 8u, nmax);
                        for (uint32_t k = k0; k < k1; k++) {
                            if (k < nl) {
                                cdf += ((S >> k) & 1ull) ? ps : el;
                                if (idx == nl && cdf > u) idx = k;
                            }
                        }
                        if (__all(!walk || idx != nl || k1 >= nl)) break;
                    }
                    if (walk) {
                        ovf = idx == nl;
                        newc = ovf ? c : idx;
                        tb = (newc == c) ? a.taboo_it : 0u;
                    }
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

// CT: the colour element, uint8_t or, for a half-word batch (chains_wide16.h), uint16_t
template <typename CT>
__global__ __launch_bounds__(64) void chains_commit_kernel(ChainArgs a, uint32_t t) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x, g = r >> 6, bit = r & 63u;
    ChainState* s = a.st + r;
    if (lane == 0u && bit == 0u) a.evcnt[((t + 1u) & 1u) * a.G + g] = 0u;   // the next sweep's counter
    if (s->done) return;
    uint32_t count = 0u;
    if (lane == 0u) {
        count = a.viol[r];
        a.viol[r] = 0u;
        if (t < a.traj_cap) a.traj[(size_t)r * a.traj_cap + t] = count;
    }
    count = (uint32_t)__shfl((int)count, 0, 64);
    if (t > a.maxRip || count <= a.z) {   // :264-269 after maxRip + 1 sweeps, :136
        if (lane == 0u) {
            s->iter = t;
            s->maxIter = t > a.maxRip ? 1u : 0u;
            s->buf = t & 1u;
            s->finalViol = count;
            s->done = 1u;
            atomicAdd(a.ndone, 1u);
        }
        return;
    }
    const uint32_t evc = min(a.evcnt[(t & 1u) * a.G + g], a.n);
    if (evc == 0u) return;
    const size_t gofs = (size_t)g * a.n * kLanes;
    const CT* Cc = reinterpret_cast<const CT*>(a.C[t & 1u]) + gofs;
    CT* Cn = reinterpret_cast<CT*>(a.C[(t + 1u) & 1u]) + gofs;
    const uint4* ev = a.evlist + (size_t)g * a.n;
    uint32_t* ring = a.ring + (size_t)r * 31u;
    uint32_t head = s->head, served = 0u;
    int64_t last = -1;
    for (;;) {   // the chain's events in ascending vertex order (:183-204 draws them in that order)
        uint32_t best = 0xFFFFFFFFu;
        for (uint32_t k = lane; k < evc; k += 64u) {
            const uint4 e = ev[k];
            const uint32_t lanes = bit < 32u ? e.y >> bit : e.z >> (bit - 32u);
            if ((lanes & 1u) && (int64_t)e.x > last) best = min(best, e.x);
        }
        for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, 64));
        if (best == 0xFFFFFFFFu) break;
        if (lane == 0u) {
            const uint32_t nc = glibc_next(ring, head) % ((uint32_t)a.ncolw[r] - 1u);   // :518, the chain's own nCol
            const size_t at = (size_t)best * kLanes + bit;
            Cn[at] = (CT)nc;
            if (a.taboo) a.taboo[gofs + at] = (nc == Cc[at]) ? a.taboo_it : 0u;   // :526
        }
        served++;
        last = (int64_t)best;
    }
    if (lane == 0u && served) {
        const uint64_t d = (((uint64_t)s->draws_hi << 32) | s->draws_lo) + served;
        s->draws_lo = (uint32_t)d;
        s->draws_hi = (uint32_t)(d >> 32);
        s->head = head;
    }
}

// tab[G * 64]: {the chain's engine seed, its UniformIntConst scaling and past, 0}, built by the host
template <typename CT>
__global__ __launch_bounds__(64) void chains_init_kernel(ChainArgs a, const uint4* __restrict__ tab) {
    const uint32_t lane = threadIdx.x, g = blockIdx.x, r = g * kLanes + lane;
    const bool live = r < a.R;
    CT* C0 = reinterpret_cast<CT*>(a.C[0]) + (size_t)g * a.n * kLanes;
    const uint4 sp = tab[r];
    UniformIntConst k;
    k.scaling = sp.y;
    k.past = sp.z;
    uint32_t x = minstd_seed_state(sp.x);
    uint64_t draws = 0;
    for (uint32_t v = 0; v < a.n; v++) {
        uint32_t col = 0u;
        if (live) {
            uint32_t rr;
            do {   // uniform_int_distribution's rejection loop (libstdc++ uniform_int_dist.h)
                x = minstd_mulmod(x, kMinstdA);
                rr = x - 1u;
                draws++;
            } while (rr >= k.past);
            col = rr / k.scaling;
        }
        C0[(size_t)v * kLanes + lane] = (CT)col;
    }
    a.xinit[r] = x;
    a.init_draws[r] = draws;
}

constexpr uint32_t kHistWaves = 4;   // waves per histogram workgroup

// Class sizes: hist[r][k] = vertices of colour k in chain r's final colouring. Grid (vertex chunks of
// `hv`, group). Colours are read as the drain reads them: lane l the dword of chains 4 (l & 15) .. +3
// of vertex l >> 4 of the wave's four, 256 B per wave-load, eight loads in flight. The chains of a
// group stop at different parities, so a lane's four chains may live in different buffers: sel has
// 0xFF in the bytes of the chains whose colouring is in buffer 1 (st[r].buf; t & 1 for a chain still
// running), and a lane loads from the buffers its chains need and merges by byte. Counts go to an LDS
// table [64 chains][64 colours] with ds_add, then one global atomic per nonzero cell and workgroup.
// The column is rotated by the chain so that the lanes of a quarter (16 chains x 4, mostly few
// distinct colours when nCol is small) spread over the banks.
__global__ __launch_bounds__(64 * kHistWaves) void chains_hist_kernel(ChainArgs a, uint32_t t, uint32_t hv) {
    __shared__ uint32_t s_h[kLanes * 64u];
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 4, i = lane & 15u, wid = threadIdx.x >> 6;
    const uint32_t g = blockIdx.y, n = a.n;
    for (uint32_t k = threadIdx.x; k < kLanes * 64u; k += 64u * kHistWaves) s_h[k] = 0u;
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
    // a wave takes 32 vertices (8 loads of 4) per turn, the workgroup's waves interleaved
    for (uint64_t vt = vb0 + 32ull * wid; vt < vend; vt += 32ull * kHistWaves) {
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
                    const uint32_t ch = 4u * i + j, col = (w[k] >> (8u * j)) & 63u;
                    if ((valid >> j) & 1u) atomicAdd(&s_h[ch * 64u + ((col + ch) & 63u)], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kLanes * 64u; k += 64u * kHistWaves) {
        const uint32_t cnt = s_h[k], ch = k >> 6, col = ((k & 63u) - ch) & 63u;
        if (cnt) atomicAdd(&a.hist[((size_t)g * kLanes + ch) * 64u + col], cnt);
    }
}

#include "chains_wide.h"
#include "chains_wide16.h"
#include "chains_tailcut.h"
#include "chains_tailcut16.h"

}  // namespace
}  // namespace mcmc

using namespace mcmc;

struct mcmc_chains {
    const mcmc_graph* g = nullptr;
    int device = 0;               // g's device: mcmc_chains_destroy must not read g (it may be gone by then)
    mcmc_params p{};
    ChainArgs a{};
    bool tiled = false;           // the sweep reads the graph's tiled layout (no CSR), else the CSR
    bool ladder = false;          // mcmc_chains_create_ladder: the per-chain instantiations of the sweep
    uint32_t mw = 0;              // mcmc_chains_create_wide / _wide16: mask words of the sweep (4, 8 / 16, 32, 64), else 0
    uint32_t esz = 1;             // bytes per colour: 2 for mcmc_chains_create_wide16 (chains_wide16.h)
    uint32_t maxncol = 0;         // the batch's largest nCol; above 64 the histogram rows are 256 wide
    std::vector<uint32_t> hist;   // get_histograms: [R][hist_cols()], valid until the next run
    bool hist_valid = false;
    size_t bytes = 0;             // of `mem`
    void* mem = nullptr;          // one device allocation behind every pointer of `a`
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t* pinned = nullptr;   // the all-done counter's host copy
    uint32_t t = 0;               // sweeps launched so far
    std::vector<uint64_t> init_draws;
    std::vector<ChainState> st;   // as of the last run
    std::vector<uint8_t> cache;   // get_coloring: one group's buffer
    int cache_g = -1, cache_buf = -1;
    // tail-cut repair (mcmc_chains_enable_repair; chains_tailcut.h)
    uint32_t repair_max = 0;      // passes at most; 0: off
    bool repaired = false;        // the repair ran (once, after the run in which the last chain stopped)
    void* rmem = nullptr;         // one device allocation behind a.vfl and every pointer of `ta`
    size_t rbytes = 0;
    TailArgs ta{};
    uint32_t* rpin = nullptr;     // a pass's counts and changed bits, pinned: [G * 64] + 2 [G]
    std::vector<uint32_t> rep_passes;   // per chain; empty until the repair ran
    std::vector<uint64_t> rep_viol;
    float repair_ms = 0.0f;
    uint32_t hist_cols() const { return esz == 2u ? 32u * mw : maxncol > 64u ? 256u : 64u; }
    uint32_t sweep_waves() const { return esz == 2u ? (uint32_t)wide16_waves((int)mw) : kSweepWaves; }
};

namespace {

// workgroups of a sweep along x: `waves` waves of vb vertices each
uint32_t chains_grid_x(const ChainArgs& a, uint32_t waves = kSweepWaves) {
    return (uint32_t)(((uint64_t)a.n + (uint64_t)a.vb * waves - 1) / ((uint64_t)a.vb * waves));
}

int chains_sync_state(mcmc_chains* c) {
    c->st.resize(c->a.R);
    MCMC_HIP_TRY(hipMemcpyAsync(c->st.data(), c->a.st, sizeof(ChainState) * c->a.R, hipMemcpyDeviceToHost, c->stream));
    MCMC_HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto& h : c->st)
        if (!h.done) {   // still running (max_sweeps): t sweeps accepted, no final count (as mcmc_run)
            h.iter = c->t;
            h.buf = c->t & 1u;
        }
    return MCMC_OK;
}

int chains_upload_windows(mcmc_chains* c, const uint32_t* w /* [R][31], nullptr: srand(1) */) {
    const uint32_t R = c->a.R;
    std::vector<uint32_t> ring((size_t)R * 31u);
    const GlibcWindow def = glibc_srand(1);
    for (uint32_t r = 0; r < R; r++) std::memcpy(&ring[(size_t)r * 31u], w ? w + (size_t)r * 31u : def.r, 31u * sizeof(uint32_t));
    int rc = chains_sync_state(c);
    if (rc) return rc;
    for (auto& s : c->st) s.head = 0u;
    MCMC_HIP_TRY(hipMemcpy(c->a.ring, ring.data(), ring.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    MCMC_HIP_TRY(hipMemcpy(c->a.st, c->st.data(), sizeof(ChainState) * R, hipMemcpyHostToDevice));
    return MCMC_OK;
}

}  // namespace

namespace {

template <bool FLAGS>
void chains_launch_sweep(mcmc_chains* c, dim3 grid, uint32_t tn) {
    const ChainArgs& a = c->a;
    if (c->esz == 2u) {   // the half-word batch (FLAGS: mcmc_chains_enable_repair16)
        if (c->mw == 64u && c->tiled)
            chains_sweep_wide16_kernel<true, 64, FLAGS><<<grid, 64 * wide16_waves(64), 0, c->stream>>>(a, c->t, tn);
        else if (c->mw == 64u)
            chains_sweep_wide16_kernel<false, 64, FLAGS><<<grid, 64 * wide16_waves(64), 0, c->stream>>>(a, c->t, tn);
        else if (c->mw == 32u && c->tiled)
            chains_sweep_wide16_kernel<true, 32, FLAGS><<<grid, 64 * wide16_waves(32), 0, c->stream>>>(a, c->t, tn);
        else if (c->mw == 32u)
            chains_sweep_wide16_kernel<false, 32, FLAGS><<<grid, 64 * wide16_waves(32), 0, c->stream>>>(a, c->t, tn);
        else if (c->tiled)
            chains_sweep_wide16_kernel<true, 16, FLAGS><<<grid, 64 * wide16_waves(16), 0, c->stream>>>(a, c->t, tn);
        else
            chains_sweep_wide16_kernel<false, 16, FLAGS><<<grid, 64 * wide16_waves(16), 0, c->stream>>>(a, c->t, tn);
    } else if (c->mw == 8u && c->tiled)
        chains_sweep_wide_kernel<true, 8, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else if (c->mw == 8u)
        chains_sweep_wide_kernel<false, 8, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else if (c->mw == 4u && c->tiled)
        chains_sweep_wide_kernel<true, 4, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else if (c->mw == 4u)
        chains_sweep_wide_kernel<false, 4, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else if (c->tiled && c->ladder)
        chains_sweep_kernel<true, true, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else if (c->tiled)
        chains_sweep_kernel<true, false, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else if (c->ladder)
        chains_sweep_kernel<false, true, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
    else
        chains_sweep_kernel<false, false, FLAGS><<<grid, 64 * kSweepWaves, 0, c->stream>>>(a, c->t, tn);
}

// c->hist: the class sizes of every chain's colouring, [R][hist_cols()]; computed on demand, kept
// until the next run
int chains_histograms(mcmc_chains* c) {
    if (c->hist_valid) return MCMC_OK;
    const ChainArgs& a = c->a;
    const uint32_t hc = c->hist_cols();
    // vertices per workgroup: 1024, more once that makes over ~1024 workgroups per group (each
    // flushes up to 64 x nCol cells); a multiple of the 32 a wave takes per turn
    uint32_t hv = (std::max(1024u, (uint32_t)(((uint64_t)a.n + 1023u) / 1024u)) + 31u) & ~31u;
    if (hc >= 256u) hv = std::min(hv, kHistWideMaxV);
    const dim3 grid((a.n + hv - 1u) / hv, a.G);
    MCMC_HIP_TRY(hipMemsetAsync(a.hist, 0, 4 * (size_t)hc * a.G * kLanes, c->stream));
    if (c->esz == 2u) {   // hc = 512, 1024 or 2048: 32, 16 or 8 chains per workgroup
        const uint32_t hc_log2 = hc == 2048u ? 11u : hc == 1024u ? 10u : 9u;
        chains_hist16_kernel<<<dim3(grid.x, a.G * (kLanes >> (14u - hc_log2))), kHist16Threads, 0, c->stream>>>(a, c->t, hv,
                                                                                                                 hc_log2);
    } else if (hc == 256u)
        chains_hist_wide_kernel<<<grid, 64 * kHistWideWaves, 0, c->stream>>>(a, c->t, hv);
    else
        chains_hist_kernel<<<grid, 64 * kHistWaves, 0, c->stream>>>(a, c->t, hv);
    MCMC_HIP_TRY(hipGetLastError());
    c->hist.resize((size_t)a.R * hc);
    MCMC_HIP_TRY(hipMemcpyAsync(c->hist.data(), a.hist, 4 * c->hist.size(), hipMemcpyDeviceToHost, c->stream));
    MCMC_HIP_TRY(hipStreamSynchronize(c->stream));
    c->hist_valid = true;
    return MCMC_OK;
}

// a pass's repair kernel of a half-word batch: the batch's table words, CSR or tiled rows
void chains_launch_repair16(mcmc_chains* c, const TailMasks& act) {
    const ChainArgs& a = c->a;
    const TailArgs& ta = c->ta;
    const uint32_t G = a.G, nc = c->maxncol;
    if (c->mw == 64u && c->tiled)
        chains_tail_repair16_kernel<true, 64><<<G * kTail16Subs, 64 * kTail16Waves, 0, c->stream>>>(a, ta, act, nc);
    else if (c->mw == 64u)
        chains_tail_repair16_kernel<false, 64><<<G * kTail16Subs, 64 * kTail16Waves, 0, c->stream>>>(a, ta, act, nc);
    else if (c->mw == 32u && c->tiled)
        chains_tail_repair16_kernel<true, 32><<<G * kTail16Subs, 64 * kTail16Waves, 0, c->stream>>>(a, ta, act, nc);
    else if (c->mw == 32u)
        chains_tail_repair16_kernel<false, 32><<<G * kTail16Subs, 64 * kTail16Waves, 0, c->stream>>>(a, ta, act, nc);
    else if (c->tiled)
        chains_tail_repair16_kernel<true, 16><<<G * kTail16Subs, 64 * kTail16Waves, 0, c->stream>>>(a, ta, act, nc);
    else
        chains_tail_repair16_kernel<false, 16><<<G * kTail16Subs, 64 * kTail16Waves, 0, c->stream>>>(a, ta, act, nc);
}

// The corrected tail cut of every chain that stopped with violators (chains_tailcut.h), after the run
// in which the last chain stopped. c->st is the state at loop exit.
int chains_repair(mcmc_chains* c) {
    const ChainArgs& a = c->a;
    const TailArgs& ta = c->ta;
    const uint32_t R = a.R, G = a.G, n = a.n;
    c->rep_passes.assign(R, 0u);
    c->rep_viol.resize(R);
    TailMasks act{}, buf1{}, par1{};
    bool any = false;
    for (uint32_t r = 0; r < R; r++) {
        const ChainState& h = c->st[r];
        c->rep_viol[r] = h.finalViol;
        if (h.buf & 1u) buf1.m[r >> 6] |= 1ull << (r & 63u);
        if (h.iter >= 1u && ((h.iter - 1u) & 1u)) par1.m[r >> 6] |= 1ull << (r & 63u);   // flags of C_{iter-1}
        if (h.finalViol > 0u) {
            act.m[r >> 6] |= 1ull << (r & 63u);
            any = true;
        }
    }
    MCMC_HIP_TRY(hipEventRecord(c->ev0, c->stream));
    const dim3 ngrid((uint32_t)(((uint64_t)n * 16u + 255u) / 256u), G);
    if (c->esz == 2u)   // the same grid: n x 16 words of 8 bytes
        chains_tail_normalise16_kernel<<<ngrid, 256, 0, c->stream>>>(a, ta, buf1, par1);
    else
        chains_tail_normalise_kernel<<<ngrid, 256, 0, c->stream>>>(a, ta, buf1, par1);
    MCMC_HIP_TRY(hipGetLastError());
    for (auto& h : c->st) h.buf = 0u;
    MCMC_HIP_TRY(hipMemcpyAsync(a.st, c->st.data(), sizeof(ChainState) * R, hipMemcpyHostToDevice, c->stream));
    MCMC_HIP_TRY(hipStreamSynchronize(c->stream));   // c->st may change under the caller from here on
    if (any && !(c->esz == 2u && a.z == 0u)) {   // a half-word batch reads no table for the identity order
        // colorIdx: the identity (:131-132); with z > 0 sorted by ascending class size (:272-278), by
        // std::sort with the reference's comparator, so ties resolve as the reference's do
        // bytes [G * 64][256]; a half-word batch: uint16_t [G * 64][ncmax] (chains_tailcut16.h)
        const uint32_t ncmax = c->maxncol;
        std::vector<uint8_t> cidx(c->esz == 2u ? 2 * (size_t)G * ncmax * kLanes : (size_t)G * kLanes * 256u, 0);
        uint16_t* cidx16 = reinterpret_cast<uint16_t*>(cidx.data());
        if (a.z > 0u) {
            int rc = chains_histograms(c);
            if (rc) return rc;
        }
        const uint32_t hc = c->hist_cols();
        std::vector<uint16_t> ncol(R);
        MCMC_HIP_TRY(hipMemcpy(ncol.data(), a.ncolw, 2 * (size_t)R, hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t k = ncol[r];
            std::vector<size_t> colorIdx(k);
            for (uint32_t i = 0; i < k; i++) colorIdx[i] = i;
            if (a.z > 0u && c->rep_viol[r] > 0u) {
                std::vector<size_t> histBins(c->hist.begin() + (size_t)r * hc, c->hist.begin() + (size_t)r * hc + k);
                std::sort(colorIdx.begin(), colorIdx.end(), [&](int i, int j) { return histBins[i] < histBins[j]; });
            }
            for (uint32_t i = 0; i < k; i++) {
                if (c->esz == 2u)
                    cidx16[(size_t)r * ncmax + i] = (uint16_t)colorIdx[i];
                else
                    cidx[(size_t)r * 256u + i] = (uint8_t)colorIdx[i];
            }
        }
        MCMC_HIP_TRY(hipMemcpyAsync(ta.cidx, cidx.data(), cidx.size(), hipMemcpyHostToDevice, c->stream));
        MCMC_HIP_TRY(hipStreamSynchronize(c->stream));   // cidx leaves scope
    }
    const dim3 cgrid(chains_grid_x(a, c->sweep_waves()), G);
    const uint32_t RP = G * kLanes;
    for (uint32_t pass = 1; any && pass <= c->repair_max; pass++) {
        chains_tail_list_kernel<<<G, kTailListThreads, 0, c->stream>>>(a, ta, act);
        if (c->esz == 2u) {   // its workgroups OR their changed bits into the groups' words
            MCMC_HIP_TRY(hipMemsetAsync(ta.chg, 0, 8 * (size_t)G, c->stream));
            chains_launch_repair16(c, act);
        } else if (c->tiled && c->maxncol > 128u)
            chains_tail_repair_kernel<true, 8><<<G, 64 * kTailWaves, 0, c->stream>>>(a, ta, act);
        else if (c->tiled)
            chains_tail_repair_kernel<true, 4><<<G, 64 * kTailWaves, 0, c->stream>>>(a, ta, act);
        else if (c->maxncol > 128u)
            chains_tail_repair_kernel<false, 8><<<G, 64 * kTailWaves, 0, c->stream>>>(a, ta, act);
        else
            chains_tail_repair_kernel<false, 4><<<G, 64 * kTailWaves, 0, c->stream>>>(a, ta, act);
        if (c->esz == 2u && c->tiled)
            chains_tail_count16_kernel<true><<<cgrid, 64 * c->sweep_waves(), 0, c->stream>>>(a, ta, act);
        else if (c->esz == 2u)
            chains_tail_count16_kernel<false><<<cgrid, 64 * c->sweep_waves(), 0, c->stream>>>(a, ta, act);
        else if (c->tiled)
            chains_tail_count_kernel<true><<<cgrid, 64 * kSweepWaves, 0, c->stream>>>(a, ta, act);
        else
            chains_tail_count_kernel<false><<<cgrid, 64 * kSweepWaves, 0, c->stream>>>(a, ta, act);
        MCMC_HIP_TRY(hipGetLastError());
        // one small copy: the R counts and the groups' changed bits (contiguous on the device)
        MCMC_HIP_TRY(hipMemcpyAsync(c->rpin, ta.cnt, 4 * (size_t)RP + 8 * (size_t)G, hipMemcpyDeviceToHost, c->stream));
        MCMC_HIP_TRY(hipStreamSynchronize(c->stream));
        uint64_t chg[kMaxGroups];
        std::memcpy(chg, c->rpin + RP, 8 * (size_t)G);
        any = false;
        for (uint32_t r = 0; r < R; r++) {
            uint64_t& m = act.m[r >> 6];
            const uint64_t bit = 1ull << (r & 63u);
            if (!(m & bit)) continue;
            c->rep_passes[r] = pass;
            c->rep_viol[r] = c->rpin[r];
            if (c->rpin[r] == 0u) {
                m &= ~bit;
            } else if (pass >= 2u && !(chg[r >> 6] & bit)) {
                // a fixed point: the same flags met the same colouring, as they will in every further pass
                // (pass 1 is excluded: its flags are those of another colouring)
                c->rep_passes[r] = c->repair_max;
                m &= ~bit;
            }
            any = any || (m & bit);
        }
    }
    MCMC_HIP_TRY(hipEventRecord(c->ev1, c->stream));
    MCMC_HIP_TRY(hipEventSynchronize(c->ev1));
    MCMC_HIP_TRY(hipEventElapsedTime(&c->repair_ms, c->ev0, c->ev1));
    c->hist_valid = false;
    c->cache_g = -1;
    c->repaired = true;
    return MCMC_OK;
}

// The batch of mcmc_chains_create (specs: nCol, epsilon of `p` and seed + r for every chain; the
// uniform sweep), of mcmc_chains_create_ladder (the caller's specs; the ladder sweep) and of
// mcmc_chains_create_wide (wide: the wide sweep, its mask words from the largest nCol) and of
// mcmc_chains_create_wide16 (esz = 2: half-word colours, the sweep of chains_wide16.h). The
// arguments other than the graph are checked by the callers.
int chains_create(const mcmc_graph* g, const mcmc_params* p, const mcmc_chain_spec* specs, uint32_t R, bool ladder,
                  bool wide, uint32_t esz, mcmc_chains** out) {
    const GraphDev& gd = g->g;
    if (gd.n == 0) return fail(MCMC_E_ARG, "chains: empty graph");
    if (gd.partial_rows)
        return fail(MCMC_E_ARG, "chains: the graph holds a row range only (mcmc_graph_er_fast_rows / _part); a batch "
                                "needs every row");
    const TiledLayout* L = nullptr;   // a generated graph: its full-range layout, read as it is
    if (!gd.row_off) {
        for (auto& tl : g->tiles)
            if (tl->v_begin == 0 && tl->v_end == gd.n) L = tl.get();
        if (!L)
            return fail(MCMC_E_ARG, "chains: the graph has neither a whole device CSR (mcmc_graph_upload / _simulate / "
                                    "_rmat) nor a full-range tiled layout (mcmc_graph_er_fast)");
    }
    MCMC_HIP_TRY(hipSetDevice(gd.device));
    const uint32_t n = gd.n, G = (R + kLanes - 1) / kLanes, RP = G * kLanes;
    const uint32_t traj_cap = (uint32_t)std::min<uint64_t>((uint64_t)p->maxRip + 2u, kTrajCapMax);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_col = up((size_t)n * kLanes * G * esz), b_tab = p->tabooIteration ? up(4 * (size_t)n * kLanes * G) : 0;
    const size_t b_ev = up(sizeof(uint4) * (size_t)n * G), b_traj = up(4 * (size_t)R * traj_cap);
    uint32_t maxncol = 0;
    for (uint32_t r = 0; r < R; r++) maxncol = std::max(maxncol, specs[r].nCol);
    const uint32_t mw = esz == 2u ? (maxncol > 1024u ? 64u : maxncol > 512u ? 32u : 16u)
                                  : wide ? (maxncol > 128u ? 8u : 4u) : 0u;
    const size_t b_hist = up(4 * (esz == 2u ? 32u * mw : maxncol > 64u ? 256u : 64u) * (size_t)RP);
    const size_t b_small = up(4 * RP) * 2 + up(8 * RP) + up(4 * 1024) + up(8 * G) + up(sizeof(ChainState) * RP) +
                           up(4 * 31 * (size_t)RP) + 256 + up(RP) + up(4 * RP) + up(sizeof(uint4) * RP) + b_hist + up(2 * RP);
    const size_t need = 2 * b_col + b_tab + b_ev + b_traj + b_small;
    size_t fr = 0, tot = 0;
    MCMC_HIP_TRY(hipMemGetInfo(&fr, &tot));
    if (need > fr)
        return fail(MCMC_E_NOMEM, "chains: " + std::to_string(need) + " bytes needed (colours 2 x " + std::to_string(b_col) +
                                      ", taboo " + std::to_string(b_tab) + ", overflow records " + std::to_string(b_ev) +
                                      ", trajectories " + std::to_string(b_traj) + "), " + std::to_string(fr) + " free");
    mcmc_chains* c = new mcmc_chains();
    c->g = g;
    c->device = gd.device;
    c->p = *p;
    hipError_t e = hipMalloc(&c->mem, need);
    if (e == hipSuccess) e = hipMemset(c->mem, 0, need);
    if (e == hipSuccess) e = hipStreamCreate(&c->stream);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->pinned), 64);
    if (e != hipSuccess) {
        mcmc_chains_destroy(c);
        return fail(e == hipErrorOutOfMemory ? MCMC_E_NOMEM : MCMC_E_HIP,
                    std::string("chains: allocation of ") + std::to_string(need) + " bytes: " + hipGetErrorString(e));
    }
    ChainArgs& a = c->a;
    uint8_t* at = static_cast<uint8_t*>(c->mem);
    auto take = [&](size_t b) { uint8_t* q = at; at += up(b); return q; };
    a.C[0] = take(b_col);
    a.C[1] = take(b_col);
    a.taboo = b_tab ? reinterpret_cast<uint32_t*>(take(b_tab)) : nullptr;
    a.evlist = reinterpret_cast<uint4*>(take(b_ev));
    a.traj = reinterpret_cast<uint32_t*>(take(b_traj));
    a.xinit = reinterpret_cast<uint32_t*>(take(4 * RP));
    a.viol = reinterpret_cast<uint32_t*>(take(4 * RP));
    a.init_draws = reinterpret_cast<uint64_t*>(take(8 * RP));
    uint32_t* powtab = reinterpret_cast<uint32_t*>(take(4 * 1024));
    a.powtab = powtab;
    a.evcnt = reinterpret_cast<uint32_t*>(take(8 * G));
    a.st = reinterpret_cast<ChainState*>(take(sizeof(ChainState) * RP));
    a.ring = reinterpret_cast<uint32_t*>(take(4 * 31 * (size_t)RP));
    a.ndone = reinterpret_cast<uint32_t*>(take(4));
    uint8_t* d_ncol = take(RP);
    float* d_eps = reinterpret_cast<float*>(take(4 * RP));
    uint4* d_itab = reinterpret_cast<uint4*>(take(sizeof(uint4) * RP));
    a.ncol = d_ncol;
    a.epsr = d_eps;
    a.hist = reinterpret_cast<uint32_t*>(take(b_hist));
    uint16_t* d_ncolw = reinterpret_cast<uint16_t*>(take(2 * RP));
    a.ncolw = d_ncolw;
    a.row_off = gd.row_off;
    a.col_idx = gd.col_idx;
    a.m = gd.m;
    if (L) {
        a.tcol = L->tcol;
        a.gbase = L->gbase;
        a.tseg = L->tseg;
        a.grp_rows = L->grp_rows;
        a.nblocks = L->nblocks;
        a.block_log2 = L->block_log2;
    }
    c->tiled = L != nullptr;
    c->ladder = ladder;
    c->mw = mw;
    c->esz = esz;
    c->maxncol = maxncol;
    c->bytes = need;
    a.n = n;
    a.R = R;
    a.G = G;
    a.nCol = p->nCol;
    a.eps = p->epsilon;
    a.taboo_it = p->tabooIteration;
    a.z = p->tailcut ? std::max<uint32_t>(50u, n / 2000u) : 0u;   // :89-97
    a.maxRip = p->maxRip;
    a.traj_cap = traj_cap;
    // vertices per wave: 16, more once the grid has ~8 waves per SIMD of a 256-CU device anyway
    a.vb = (uint32_t)std::min<uint64_t>(64u, std::max<uint64_t>(16u, ((uint64_t)n * G + 8191u) / 8192u));
    if (const char* s = getenv("MCMC_CHAINS_VB")) a.vb = std::min(1024u, std::max(1u, (uint32_t)atoi(s)));
    std::vector<uint32_t> tab(1024);
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t b = minstd_pow(kMinstdA, 1ull << (8 * k));
        tab[k * 256] = 1u;
        for (uint32_t j = 1; j < 256; j++) tab[k * 256 + j] = minstd_mulmod(tab[k * 256 + j - 1], b);
    }
    e = hipMemcpy(powtab, tab.data(), 4096, hipMemcpyHostToDevice);
    // per-chain tables: nCol, epsilon, and the init kernel's {seed, UniformIntConst}
    std::vector<uint8_t> h_ncol(RP, 0);
    std::vector<uint16_t> h_ncolw(RP, 0);
    std::vector<float> h_eps(RP, 0.0f);
    std::vector<uint4> h_itab(RP, make_uint4(1u, 1u, 1u, 0u));
    for (uint32_t r = 0; r < R; r++) {
        const UniformIntConst k = uniform_int_const(specs[r].nCol);
        h_ncol[r] = (uint8_t)specs[r].nCol;
        h_ncolw[r] = (uint16_t)specs[r].nCol;
        h_eps[r] = specs[r].epsilon;
        h_itab[r] = make_uint4(specs[r].seed, k.scaling, k.past, 0u);
    }
    if (e == hipSuccess) e = hipMemcpy(d_ncol, h_ncol.data(), RP, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_ncolw, h_ncolw.data(), 2 * (size_t)RP, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_eps, h_eps.data(), 4 * (size_t)RP, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_itab, h_itab.data(), sizeof(uint4) * (size_t)RP, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (esz == 2u)
            chains_init_kernel<uint16_t><<<G, 64, 0, c->stream>>>(a, d_itab);
        else
            chains_init_kernel<uint8_t><<<G, 64, 0, c->stream>>>(a, d_itab);
        e = hipGetLastError();
    }
    c->init_draws.resize(RP);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->init_draws.data(), a.init_draws, 8 * (size_t)RP, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int rc = e == hipSuccess ? chains_upload_windows(c, nullptr) : fail(MCMC_E_HIP, std::string("chains init: ") + hipGetErrorString(e));
    if (rc) {
        mcmc_chains_destroy(c);
        return rc;
    }
    *out = c;
    return MCMC_OK;
}

}  // namespace

namespace {

// mcmc_chains_enable_repair / _repair16 after their checks: the pass cap and, once, the flag words, the
// lists and the colour-order table (bytes [G * 64][256]; a half-word batch: uint16_t [G * 64][largest nCol])
int chains_enable_repair(mcmc_chains* c, uint32_t max_passes) {
    MCMC_HIP_TRY(hipSetDevice(c->device));
    c->repair_max = max_passes;
    if (!max_passes || c->rmem) return MCMC_OK;
    const ChainArgs& a = c->a;
    const size_t n = a.n, G = a.G, RP = G * kLanes;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_vfl = up(16 * n * G), b_fl = up(8 * n * G), b_list = up(4 * n * G), b_len = up(4 * G),
                 b_cidx = up(c->esz == 2u ? 2 * kLanes * (size_t)c->maxncol * G : 256 * RP), b_cnt = up(4 * RP + 8 * G);
    const size_t need = b_vfl + b_fl + b_list + b_len + b_cidx + b_cnt;
    hipError_t e = hipMalloc(&c->rmem, need);
    if (e == hipSuccess) e = hipMemset(c->rmem, 0, need);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->rpin), 4 * RP + 8 * G);
    if (e != hipSuccess) {
        if (c->rmem) (void)hipFree(c->rmem);
        c->rmem = nullptr;
        c->repair_max = 0;
        return fail(e == hipErrorOutOfMemory ? MCMC_E_NOMEM : MCMC_E_HIP,
                    std::string("chains: tail-cut repair needs ") + std::to_string(need) + " bytes (sweep flags " +
                        std::to_string(b_vfl) + ", pass flags " + std::to_string(b_fl) + ", lists " + std::to_string(b_list) +
                        ", colour order " + std::to_string(b_cidx) + "): " + hipGetErrorString(e));
    }
    uint8_t* at = static_cast<uint8_t*>(c->rmem);
    auto take = [&](size_t b) { uint8_t* q = at; at += b; return q; };
    c->a.vfl = reinterpret_cast<uint64_t*>(take(b_vfl));
    c->ta.fl = reinterpret_cast<uint64_t*>(take(b_fl));
    c->ta.list = reinterpret_cast<uint32_t*>(take(b_list));
    c->ta.listlen = reinterpret_cast<uint32_t*>(take(b_len));
    c->ta.cidx = take(b_cidx);
    c->ta.cnt = reinterpret_cast<uint32_t*>(take(b_cnt));
    c->ta.chg = reinterpret_cast<uint64_t*>(c->ta.cnt + RP);   // 4 RP is a multiple of 8
    c->rbytes = need;
    return MCMC_OK;
}

}  // namespace

extern "C" {

int mcmc_chains_create(const mcmc_graph* g, const mcmc_params* p, uint32_t R, mcmc_chains** out) {
    if (!g || !p || !out) return fail(MCMC_E_ARG, "NULL argument");
    *out = nullptr;
    if (p->nCol < 2 || p->nCol > 64)
        return fail(MCMC_E_ARG, "chains: 2 <= nCol <= 64 (one 64-bit occupancy mask per lane), got " + std::to_string(p->nCol));
    if (R < 1 || R > kMaxChains) return fail(MCMC_E_ARG, "chains: 1 <= R <= 1024, got " + std::to_string(R));
    std::vector<mcmc_chain_spec> specs(R);
    for (uint32_t r = 0; r < R; r++) specs[r] = mcmc_chain_spec{p->nCol, p->seed + r, p->epsilon, 0u};
    return chains_create(g, p, specs.data(), R, false, false, 1u, out);
}

int mcmc_chains_create_ladder(const mcmc_graph* g, const mcmc_params* p, const mcmc_chain_spec* specs, uint32_t R,
                              mcmc_chains** out) {
    if (!g || !p || !specs || !out) return fail(MCMC_E_ARG, "NULL argument");
    *out = nullptr;
    if (R < 1 || R > kMaxChains) return fail(MCMC_E_ARG, "chains: 1 <= R <= 1024, got " + std::to_string(R));
    for (uint32_t r = 0; r < R; r++) {
        if (specs[r].nCol < 2 || specs[r].nCol > 64)
            return fail(MCMC_E_ARG, "chains: chain " + std::to_string(r) + ": 2 <= nCol <= 64 (one 64-bit occupancy mask "
                                    "per lane), got " + std::to_string(specs[r].nCol));
        if (specs[r].reserved != 0)
            return fail(MCMC_E_ARG, "chains: chain " + std::to_string(r) + ": reserved must be 0");
    }
    return chains_create(g, p, specs, R, true, false, 1u, out);
}

int mcmc_chains_create_wide(const mcmc_graph* g, const mcmc_params* p, const mcmc_chain_spec* specs, uint32_t R,
                            mcmc_chains** out) {
    if (!g || !p || !out) return fail(MCMC_E_ARG, "NULL argument");
    *out = nullptr;
    if (R < 1 || R > kMaxChains) return fail(MCMC_E_ARG, "chains: 1 <= R <= 1024, got " + std::to_string(R));
    std::vector<mcmc_chain_spec> sp(R);
    for (uint32_t r = 0; r < R; r++) {
        sp[r] = specs ? specs[r] : mcmc_chain_spec{p->nCol, p->seed + r, p->epsilon, 0u};
        if (sp[r].nCol < 2 || sp[r].nCol > 256)
            return fail(MCMC_E_ARG, "chains: chain " + std::to_string(r) + ": 2 <= nCol <= 256 (the wide sweep's occupancy "
                                    "table), got " + std::to_string(sp[r].nCol));
        if (sp[r].reserved != 0)
            return fail(MCMC_E_ARG, "chains: chain " + std::to_string(r) + ": reserved must be 0");
    }
    return chains_create(g, p, sp.data(), R, true, true, 1u, out);
}

int mcmc_chains_create_wide16(const mcmc_graph* g, const mcmc_params* p, const mcmc_chain_spec* specs, uint32_t R,
                              mcmc_chains** out) {
    if (!g || !p || !out) return fail(MCMC_E_ARG, "NULL argument");
    *out = nullptr;
    if (R < 1 || R > kMaxChains) return fail(MCMC_E_ARG, "chains: 1 <= R <= 1024, got " + std::to_string(R));
    std::vector<mcmc_chain_spec> sp(R);
    for (uint32_t r = 0; r < R; r++) {
        sp[r] = specs ? specs[r] : mcmc_chain_spec{p->nCol, p->seed + r, p->epsilon, 0u};
        if (sp[r].nCol < 2 || sp[r].nCol > 2048)
            return fail(MCMC_E_ARG, "chains: chain " + std::to_string(r) + ": 2 <= nCol <= 2048 (the half-word sweep's "
                                    "occupancy table), got " + std::to_string(sp[r].nCol));
        if (sp[r].reserved != 0)
            return fail(MCMC_E_ARG, "chains: chain " + std::to_string(r) + ": reserved must be 0");
    }
    return chains_create(g, p, sp.data(), R, true, true, 2u, out);
}

int mcmc_chains_get_info(mcmc_chains* c, uint64_t out[8]) {
    if (!c || !out) return fail(MCMC_E_ARG, "NULL argument");
    const uint64_t w[8] = {c->tiled ? 1u : 0u, c->bytes, c->a.vb, c->a.G, chains_grid_x(c->a, c->sweep_waves()), c->ladder ? 1u : 0u, c->mw,
                           (uint64_t)((double)c->repair_ms * 1000.0 + 0.5)};
    std::memcpy(out, w, sizeof(w));
    return MCMC_OK;
}

int mcmc_chains_set_glibc_windows(mcmc_chains* c, const uint32_t* windows) {
    if (!c || !windows) return fail(MCMC_E_ARG, "NULL argument");
    MCMC_HIP_TRY(hipSetDevice(c->g->g.device));
    return chains_upload_windows(c, windows);
}

int mcmc_chains_set_tailcut_repair(mcmc_chains* c, uint32_t max_passes) {
    if (!c) return fail(MCMC_E_ARG, "NULL context");
    if (max_passes) return fail(MCMC_E_ARG, "chains: tail-cut repair is not supported (run the chain with mcmc_run)");
    return MCMC_OK;
}

int mcmc_chains_enable_repair(mcmc_chains* c, uint32_t max_passes) {
    if (!c) return fail(MCMC_E_ARG, "NULL context");
    if (c->t != 0u) return fail(MCMC_E_ARG, "chains: mcmc_chains_enable_repair after a run has started (the sweeps so far kept no flags)");
    if (max_passes && c->esz == 2u)
        return fail(MCMC_E_ARG, "chains: mcmc_chains_enable_repair reads byte colours: a half-word batch "
                                "(mcmc_chains_create_wide16) is repaired by mcmc_chains_enable_repair16");
    return chains_enable_repair(c, max_passes);
}

int mcmc_chains_enable_repair16(mcmc_chains* c, uint32_t max_passes) {
    if (!c) return fail(MCMC_E_ARG, "NULL context");
    if (c->esz != 2u)
        return fail(MCMC_E_ARG, "chains: mcmc_chains_enable_repair16 reads 16-bit colours: a batch other than "
                                "mcmc_chains_create_wide16's is repaired by mcmc_chains_enable_repair");
    if (c->t != 0u) return fail(MCMC_E_ARG, "chains: mcmc_chains_enable_repair16 after a run has started (the sweeps so far kept no flags)");
    return chains_enable_repair(c, max_passes);
}

int mcmc_chains_get_glibc_windows(mcmc_chains* c, uint32_t* windows) {
    if (!c || !windows) return fail(MCMC_E_ARG, "NULL argument");
    MCMC_HIP_TRY(hipSetDevice(c->g->g.device));
    int rc = chains_sync_state(c);
    if (rc) return rc;
    std::vector<uint32_t> ring((size_t)c->a.R * 31u);
    MCMC_HIP_TRY(hipMemcpy(ring.data(), c->a.ring, ring.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < c->a.R; r++)
        for (uint32_t i = 0; i < 31; i++) windows[(size_t)r * 31u + i] = ring[(size_t)r * 31u + (c->st[r].head + i) % 31u];
    return MCMC_OK;
}

int mcmc_chains_run(mcmc_chains* c, uint32_t max_sweeps, mcmc_run_stats* stats) {
    if (!c) return fail(MCMC_E_ARG, "NULL context");
    MCMC_HIP_TRY(hipSetDevice(c->g->g.device));
    const ChainArgs& a = c->a;
    // at most maxRip + 2 sweeps in all: the last one only counts (:264-269)
    const uint64_t cap = (uint64_t)a.maxRip + 2u;
    const uint64_t left = cap > c->t ? cap - c->t : 0u;
    const uint32_t total = (uint32_t)(max_sweeps ? std::min<uint64_t>(max_sweeps, left) : left);
    const dim3 grid(chains_grid_x(a, c->sweep_waves()), a.G);
    c->cache_g = -1;
    c->hist_valid = false;
    MCMC_HIP_TRY(hipEventRecord(c->ev0, c->stream));
    // The all-done counter is read every kPollSweeps sweeps: a read drains the stream (~20 us), a
    // sweep + commit pair of a small graph is ~10 us, and the at most kPollSweeps - 1 pairs launched
    // past the last stop return at their first instruction.
    for (uint32_t k = 0; k < total;) {
        const uint32_t b = std::min(kPollSweeps, total - k);
        for (uint32_t j = 0; j < b; j++, c->t++) {
            const uint32_t tn = (uint32_t)(((uint64_t)c->t * a.n) % kMinstdN);
            if (c->repair_max)
                chains_launch_sweep<true>(c, grid, tn);
            else
                chains_launch_sweep<false>(c, grid, tn);
            if (c->esz == 2u)
                chains_commit_kernel<uint16_t><<<a.R, 64, 0, c->stream>>>(a, c->t);
            else
                chains_commit_kernel<uint8_t><<<a.R, 64, 0, c->stream>>>(a, c->t);
        }
        MCMC_HIP_TRY(hipGetLastError());
        k += b;
        MCMC_HIP_TRY(hipMemcpyAsync(c->pinned, a.ndone, 4, hipMemcpyDeviceToHost, c->stream));
        MCMC_HIP_TRY(hipStreamSynchronize(c->stream));
        if (*c->pinned >= a.R) break;
    }
    MCMC_HIP_TRY(hipEventRecord(c->ev1, c->stream));
    MCMC_HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    MCMC_HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    int rc = chains_sync_state(c);
    if (rc) return rc;
    // the tail cut, once, after the run in which the last chain stopped (a run cut short by max_sweeps
    // repairs nothing); loopMs stays the sweep loop's time
    if (c->repair_max && !c->repaired &&
        std::all_of(c->st.begin(), c->st.end(), [](const ChainState& h) { return h.done != 0u; })) {
        rc = chains_repair(c);
        if (rc) return rc;
    }
    for (uint32_t r = 0; r < a.R; r++) {
        const ChainState& h = c->st[r];
        if (!stats) break;
        mcmc_run_stats s{};
        s.iter = h.iter;
        s.maxIterReached = h.done ? (int32_t)h.maxIter : 0;
        s.finalViol = h.done ? h.finalViol : ~0ull;
        s.trajLen = std::min<uint64_t>((uint64_t)h.iter + (h.done ? 1u : 0u), a.traj_cap);
        s.glibcDraws = ((uint64_t)h.draws_hi << 32) | h.draws_lo;
        s.initDraws = c->init_draws[r];
        s.loopMs = ms;
        s.sweepsRun = h.iter + (h.done ? 1u : 0u);
        if (c->repaired) {
            s.finalViol = c->rep_viol[r];
            s.tailcutPasses = c->rep_passes[r];
        }
        stats[r] = s;
    }
    return MCMC_OK;
}

int mcmc_chains_get_coloring(mcmc_chains* c, uint32_t r, uint32_t* out) {
    if (!c || !out) return fail(MCMC_E_ARG, "NULL argument");
    if (r >= c->a.R) return fail(MCMC_E_ARG, "chain index out of range");
    MCMC_HIP_TRY(hipSetDevice(c->g->g.device));
    const uint32_t n = c->a.n;
    if (c->st.size() != c->a.R) {
        int rc = chains_sync_state(c);
        if (rc) return rc;
    }
    const int g = (int)(r / kLanes), buf = (int)c->st[r].buf;
    if (g != c->cache_g || buf != c->cache_buf) {   // one download serves the group's chains
        c->cache.resize((size_t)n * kLanes * c->esz);
        MCMC_HIP_TRY(hipMemcpy(c->cache.data(), c->a.C[buf] + (size_t)g * n * kLanes * c->esz, c->cache.size(),
                               hipMemcpyDeviceToHost));
        c->cache_g = g;
        c->cache_buf = buf;
    }
    if (c->esz == 2u) {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(c->cache.data());
        for (uint32_t v = 0; v < n; v++) out[v] = h[(size_t)v * kLanes + (r % kLanes)];
    } else {
        for (uint32_t v = 0; v < n; v++) out[v] = c->cache[(size_t)v * kLanes + (r % kLanes)];
    }
    return MCMC_OK;
}

int mcmc_chains_get_histograms_n(mcmc_chains* c, uint32_t* out, uint32_t cols) {
    if (!c || !out) return fail(MCMC_E_ARG, "NULL argument");
    if (cols < c->maxncol)
        return fail(MCMC_E_ARG, "chains: histogram rows of " + std::to_string(cols) + " colours, the batch's largest nCol is " +
                                    std::to_string(c->maxncol));
    MCMC_HIP_TRY(hipSetDevice(c->g->g.device));
    const ChainArgs& a = c->a;
    const uint32_t hc = c->hist_cols();
    if (int rc = chains_histograms(c)) return rc;
    const uint32_t k = std::min(cols, hc);   // columns past the kernel's row are colours no chain has
    for (uint32_t r = 0; r < a.R; r++) {
        std::memcpy(out + (size_t)r * cols, c->hist.data() + (size_t)r * hc, 4 * (size_t)k);
        std::memset(out + (size_t)r * cols + k, 0, 4 * (size_t)(cols - k));
    }
    return MCMC_OK;
}

int mcmc_chains_get_histograms(mcmc_chains* c, uint32_t* out) {
    if (!c || !out) return fail(MCMC_E_ARG, "NULL argument");
    if (c->maxncol > 64u)
        return fail(MCMC_E_ARG, "chains: the batch's largest nCol is " + std::to_string(c->maxncol) +
                                    ": its histogram rows do not fit 64 columns (mcmc_chains_get_histograms_n)");
    return mcmc_chains_get_histograms_n(c, out, 64u);
}

int mcmc_chains_get_trajectory(mcmc_chains* c, uint32_t r, uint64_t* out, uint64_t cap, uint64_t* len) {
    if (!c || !len) return fail(MCMC_E_ARG, "NULL argument");
    if (r >= c->a.R) return fail(MCMC_E_ARG, "chain index out of range");
    MCMC_HIP_TRY(hipSetDevice(c->g->g.device));
    if (c->st.size() != c->a.R) {
        int rc = chains_sync_state(c);
        if (rc) return rc;
    }
    const ChainState& h = c->st[r];
    const uint64_t have = std::min<uint64_t>(h.done ? (uint64_t)h.iter + 1u : c->t, c->a.traj_cap);
    *len = have;
    const uint64_t k = out ? std::min(have, cap) : 0u;
    if (k) {
        std::vector<uint32_t> tmp(k);
        MCMC_HIP_TRY(hipMemcpy(tmp.data(), c->a.traj + (size_t)r * c->a.traj_cap, 4 * k, hipMemcpyDeviceToHost));
        for (uint64_t j = 0; j < k; j++) out[j] = tmp[j];
    }
    return MCMC_OK;
}

void mcmc_chains_destroy(mcmc_chains* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->mem) (void)hipFree(c->mem);
    if (c->rmem) (void)hipFree(c->rmem);
    if (c->rpin) (void)hipHostFree(c->rpin);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

}  // extern "C"
