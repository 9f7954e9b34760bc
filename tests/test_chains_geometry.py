"""Launch geometry of the batched chains (csrc/chains.hip, csrc/chains_wide.h): the paths the production graphs
take on every sweep and the ~300-vertex cases of the sibling modules never reach -- vertices per wave other than
16 (MCMC_CHAINS_VB, and the host's own rule above 16), a layout group that ends inside a wave's block in all four
tiled sweeps, histogram kernels over many workgroups, wide sweeps over two column blocks, the tiled drain's
second directory round, 16 chain groups, a graph smaller than a workgroup, a last wave of one vertex.

Every comparison is exact, as in the sibling modules: chain r equals the oracle's run of its own (nCol_r, eps_r,
seed_r) started at srand(S) -- colouring, full trajectory, iter, maxIterReached, finalViol, glibcDraws, initDraws
and the advanced glibc window -- and its device histogram equals the bincount of the oracle's colouring."""
import time
from functools import lru_cache

import numpy as np
import pytest

import oracle_ref as O
from test_chains import S
from test_chains_tiled import graph as er_graph
from test_chains_wide import EPS10, csr as named_csr, specs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip_lib):
    import mcmc_colorer_amd.colorer as M

    return M


@lru_cache(maxsize=None)
def csr(name):
    """A named CSR, or ("er", n, p): the CSR the generated graph downloads."""
    if isinstance(name, tuple):
        return er_graph(*name[1:])[1:]
    if name == "sparse":   # three histogram workgroups of 1024 vertices, the last with 483 (no multiple of 32)
        O.srand(1)
        return O.setup_rnd2(2531, 0.004)
    if name == "small":    # fewer vertices than one sweep workgroup's 64: waves of 16, 16, 8 and an idle one
        O.srand(1)
        return O.setup_rnd2(40, 0.2)
    if name == "n17":      # G(16, 0.3) and the isolated vertex 16: the second wave owns that one vertex
        O.srand(1)
        off, idx = O.setup_rnd2(16, 0.3)
        return np.append(off, off[-1]), idx
    if name == "n1":       # a single isolated vertex: the drain's id clamp n - 1 is 0
        return np.zeros(2, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    return named_csr(name)   # "er", "fill", "iso" and the graphs of test_chains.py


def device_graph(M, name):
    if name == "er" or isinstance(name, tuple):
        return er_graph(*(name[1:] if isinstance(name, tuple) else (300, 0.1)))[0]
    return M.Graph.from_csr(*csr(name))


@lru_cache(maxsize=None)
def oracle(name, spec, maxRip, taboo, sweep_limit=0, nthreads=1):
    off, idx = csr(name)
    O.srand(S)
    return O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                      sweep_limit=sweep_limit, nthreads=nthreads)


def uniform(ncol, eps, seed, R):
    return specs([ncol] * R, eps, [seed + r for r in range(R)])


def batch(M, g, kind, sp, maxRip, taboo=0):
    """kind "uniform": mcmc_chains_create (sp is uniform(...)); "ladder" / "wide": the caller's specs."""
    if kind == "uniform":
        params = M.ColoringMCMCParams(nCol=sp[0][0], epsilon=sp[0][1], maxRip=maxRip, tabooIteration=taboo)
        return M.ColoringMCMCChains(g, params, sp[0][2], len(sp), glibc=M.GlibcRand(S, 0))
    params = M.ColoringMCMCParams(nCol=0, maxRip=maxRip, tabooIteration=taboo)
    return M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide=kind == "wide")


# info()[0], [5], [6] of a batch: adjacency source, ladder flag, mask words
def code_object(kind, tiled, sp):
    return [int(tiled), int(kind != "uniform"), 0 if kind != "wide" else 8 if max(s[0] for s in sp) > 128 else 4]


def assert_info(ch, n, kind, tiled, sp, vb):
    info = ch.info()
    assert [info[0], info[5], info[6]] == code_object(kind, tiled, sp), info
    assert info[2] == vb and info[3] == (len(sp) + 63) // 64 and info[4] == -(-n // (4 * vb)), info


def check(M, ch, sp, refs, max_sweeps=0):
    """test_chains_wide.check for either histogram width, plus the empty columns past a chain's nCol."""
    stats, cols, trajs, hist = ch.run(max_sweeps), ch.colorings(), ch.trajectories(), ch.histograms()
    width = 256 if ch.wide else 64
    assert hist.shape == (len(sp), width)
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        assert trajs[r].tolist() == (ref.traj[:max_sweeps] if max_sweeps else ref.traj).tolist(), f"chain {r}"
        assert (st.iter, st.glibcDraws, st.initDraws) == (ref.res.iter, ref.res.glibcDraws, ref.res.initDraws), r
        if not max_sweeps:
            assert (bool(st.maxIterReached), st.finalViol) == (bool(ref.res.maxIterReached), ref.res.finalViol), r
        assert np.array_equal(ch.glibc[r].window, M.GlibcRand(S, ref.res.glibcDraws).window), r
        assert hist[r].tolist() == np.bincount(ref.colors, minlength=width).tolist(), r
        assert not hist[r, sp[r][0]:].any(), r
    return stats


# ---- 1. vertices per wave, over all eight sweep code objects -----------------------------------------------------
WIDTHS10 = [2, 33, 64, 65, 96, 97, 128, 129, 255, 256]   # every word boundary of the wide table
SEEDS10 = [7, 12, 4099, 5, 58, 302, 9, 77, 3, 100]
# id: sweep kind, graph, (nCol, eps, seed) per chain, maxRip, taboo
SWEEPS = {
    "uniform-csr": ("uniform", "hub", uniform(16, 1e-8, 5, 5), 250, 2),   # degree 100 and degree 0
    "ladder-csr": ("ladder", "rnd", specs([2, 16, 33, 64, 17], [1e-8, 1e-6, 1e-8, 1e-4, 1e-8], [7, 302, 12, 4099, 58]), 40, 0),
    "uniform-tiled": ("uniform", "er", uniform(16, 1e-8, 3, 5), 250, 0),
    "ladder-tiled": ("ladder", "er", specs([16, 4, 64, 33, 25], 1e-8, [3, 90, 4, 17, 8]), 250, 0),
    "wide4-csr": ("wide", "fill", specs([65, 70, 80], [1e-8, 1e-6, 1e-8], [21, 44, 13]), 12, 0),   # the row scan's early exit
    "wide8-csr": ("wide", "rnd", specs(WIDTHS10, EPS10, SEEDS10), 30, 0),
    "wide4-tiled": ("wide", "er", specs([16, 65, 128], 1e-8, [3, 90, 4]), 30, 0),
    "wide8-tiled": ("wide", "er", specs([16, 65, 130], 1e-8, [3, 90, 4]), 30, 0),
}
# eps = 3.3e6: every vertex of colour 0 that does not violate overflows, every sweep. The records of a vertex
# range now come from other waves and workgroups, and the commit still has to serve them in ascending vertex order.
# The wide batch keeps the widths of test_chains_ladder's case: an overflow moves its vertex out of colour 0, so a
# chain draws about n / nCol times in all, and above ~30 colours that is fewer draws than sweeps on this graph.
OVERFLOWS = {
    "uniform-csr": ("uniform", "rnd", uniform(16, 3.3e6, 100, 5), 6, 2),
    "wide4-csr": ("wide", "rnd", specs([16, 7, 24, 30, 9], 3.3e6, [100, 3, 77, 100, 3]), 6, 2),
}
# vb = 5: waves begin and end inside the generated graph's layout groups of 32 rows (all four tiled sweeps change
# group in mid-block); vb = 1024: the whole graph in wave 0 of one workgroup, three waves idle; vb = 1: ~75 workgroups
VBS = [1, 5, 64, 1024]


def run_with_vb(M, monkeypatch, case, vb, overflow):
    kind, name, sp, maxRip, taboo = case
    refs = [oracle(name, s, maxRip, taboo) for s in sp]
    if overflow:   # some sweep serves several events of every chain
        assert all(r.res.glibcDraws > r.res.iter for r in refs), [(r.res.glibcDraws, r.res.iter) for r in refs]
    monkeypatch.setenv("MCMC_CHAINS_VB", str(vb))   # read by getenv when the batch is created
    ch = batch(M, device_graph(M, name), kind, sp, maxRip, taboo)
    assert_info(ch, len(csr(name)[0]) - 1, kind, name == "er", sp, vb)
    check(M, ch, sp, refs)


@pytest.mark.parametrize("vb", VBS)
@pytest.mark.parametrize("sweep", SWEEPS)
def test_block_sizes(M, monkeypatch, sweep, vb):
    run_with_vb(M, monkeypatch, SWEEPS[sweep], vb, False)


@pytest.mark.parametrize("vb", [5, 64])
@pytest.mark.parametrize("sweep", OVERFLOWS)
def test_block_sizes_with_overflows_every_sweep(M, monkeypatch, sweep, vb):
    run_with_vb(M, monkeypatch, OVERFLOWS[sweep], vb, True)


def hidden_exit_rows(name, sp, refs):
    """Rows of the oracle's initial colourings at which, after some whole chunk of 64 neighbours short of the row's
    end, every chain has seen all of its colours below 32 (mask word 0), some chain has not seen all of its colours,
    and that chain's missing colours are still to come: an exit test that reads word 0 alone leaves the row early
    and gets that chain's free-colour count wrong."""
    off, idx = (a.astype(np.int64) for a in csr(name))
    rows = []
    for v in range(len(off) - 1):
        nb = idx[off[v]:off[v + 1]]
        for e in range(64, len(nb), 64):
            seen = [np.unique(ref.init[nb[:e]]) for ref in refs]
            if all((c < 32).sum() == min(32, s[0]) for c, s in zip(seen, sp)):
                if any(len(c) < s[0] and len(np.setdiff1d(ref.init[nb[e:]], c)) for c, s, ref in zip(seen, sp, refs)):
                    rows.append(v)
                break   # the first chunk at which word 0 is full decides
    return rows


# degree ~540 over one column block: rows of nine chunks; 128 and 130 colours fill word 0 chunks before the rest
@pytest.mark.parametrize("ncols,mw", [([128, 65, 16], 4), ([130, 65, 16], 8)])
def test_wide_tiled_exit_test_reads_every_mask_word(M, ncols, mw):
    name, sp, maxRip = ("er", 600, 0.9), specs(ncols, 1e-8, [3, 90, 4]), 4
    refs = [oracle(name, s, maxRip, 0) for s in sp]
    assert len(hidden_exit_rows(name, sp, refs)) >= 10
    ch = batch(M, device_graph(M, name), "wide", sp, maxRip)
    assert_info(ch, 600, "wide", True, sp, 16)
    assert ch.info()[6] == mw
    check(M, ch, sp, refs)


# ---- 2. the host's own vb above 16, wide sweeps over two column blocks, histograms over 69 workgroups -------------
BIG = ("er", 70000, 3e-4)   # two column blocks of 65536 ids


def two_blocks(off, idx):
    """test_chains_tiled's "blocks": an id in block 1, and a row whose block-1 segment is empty."""
    rowmax = np.maximum.reduceat(idx, off[:-1].astype(np.int64).clip(max=len(idx) - 1))
    return idx.max() >= 65536 and (rowmax[np.diff(off) > 0] < 65536).any()


def host_vb(n, R):
    return min(64, max(16, (n * ((R + 63) // 64) + 8191) // 8192))


def test_host_block_size_above_16_ends_layout_groups_in_mid_block(M):
    n = BIG[1]
    g = device_graph(M, BIG)
    grp_rows = M.ColoringMCMC(g, M.GPURand(n, 1, M.GlibcRand(1)), M.ColoringMCMCParams(nCol=16)).info()["grp_rows"]
    # R = 65: two chain groups, the second of a single chain, vb = 18. Were grp_rows a multiple of it on the device
    # at hand, a third or fourth group gives vb = 26 or 35.
    R = next(R for R in (65, 129, 193) if grp_rows % host_vb(n, R))
    assert grp_rows > 0 and 16 < host_vb(n, R) < 64 and grp_rows % host_vb(n, R), (grp_rows, R)
    sp = uniform(16, 1e-8, 4, R)
    refs = [oracle(BIG, s, 250, 0, 3, 4) for s in sp]   # four oracle threads: the same run, sooner
    assert two_blocks(*csr(BIG))
    assert not any(r.res.iter < 3 for r in refs)   # every chain still runs: the histograms read buffer 3 & 1
    ch = batch(M, g, "uniform", sp, 250)
    assert_info(ch, n, "uniform", True, sp, host_vb(n, R))
    assert (R, ch.info()[2]) in ((65, 18), (129, 26), (193, 35))
    check(M, ch, sp, refs, max_sweeps=3)   # 69 histogram workgroups per group


def test_wide_sweep_over_two_column_blocks(M):
    n, sp = BIG[1], specs([65, 130, 16], 1e-8, [3, 90, 4])
    refs = [oracle(BIG, s, 250, 0, 3, 4) for s in sp]   # four oracle threads: the same run, sooner
    assert two_blocks(*csr(BIG))
    assert not any(r.res.iter < 3 for r in refs)
    ch = batch(M, device_graph(M, BIG), "wide", sp, 250)
    assert_info(ch, n, "wide", True, sp, 16)
    check(M, ch, sp, refs, max_sweeps=3)   # the 256-column histogram kernel over 69 workgroups


# ---- 3. histograms of stopped chains across workgroups (CSR) -----------------------------------------------------
# epsilon, maxRip and the seeds come from a CPU search with the oracle alone: at 1e-8 every chain of this sparse
# graph stops within three sweeps; at these epsilons none stops before sweep 3, chains stop on even and on odd
# sweeps (in either buffer), and others run into the cap.
STOPPED = {
    "narrow": ("ladder", specs([8 + r % 57 for r in range(70)], 2e-4, [4 + 2 * r for r in range(70)]), 24),
    "wide": ("wide", specs([2, 64, 65, 129, 255, 256], 1e-4, [1, 1, 2, 1, 3, 6]), 24),
}


@pytest.mark.parametrize("case", STOPPED)
def test_histograms_of_stopped_chains_over_three_workgroups(M, case):
    kind, sp, maxRip = STOPPED[case]
    refs = [oracle("sparse", s, maxRip, 0) for s in sp]
    stops = [r.res.iter for r in refs if not r.res.maxIterReached]
    assert {i & 1 for i in stops} == {0, 1} and any(r.res.maxIterReached for r in refs), stops
    assert min(r.res.iter for r in refs) >= 3, stops
    n = len(csr("sparse")[0]) - 1
    assert (n + 1023) // 1024 == 3 and n % 1024 % 32
    ch = batch(M, device_graph(M, "sparse"), kind, sp, maxRip)
    assert_info(ch, n, kind, False, sp, 16)
    check(M, ch, sp, [oracle("sparse", s, maxRip, 0, 3) for s in sp], max_sweeps=3)   # all chains still running
    check(M, ch, sp, refs)


# ---- 4. batch-shape edges ---------------------------------------------------------------------------------------
def test_1024_chains_on_a_graph_smaller_than_a_workgroup(M):
    sp = uniform(4, 1e-8, 3, 1024)
    refs = [oracle("small", s, 10, 2) for s in sp]
    ch = batch(M, device_graph(M, "small"), "uniform", sp, 10, taboo=2)
    assert_info(ch, 40, "uniform", False, sp, 16)   # one workgroup: waves of 16, 16 and 8 vertices, wave 3 idle
    assert ch.info()[3:5] == [16, 1]
    check(M, ch, sp, refs)


def test_wide_ladder_of_three_groups_the_last_of_two_chains(M):
    sp = specs([2 + (r * 37) % 255 for r in range(130)], 1e-8, [3 + 2 * r for r in range(130)])
    refs = [oracle("rnd", s, 12, 0) for s in sp]
    ch = batch(M, device_graph(M, "rnd"), "wide", sp, 12)
    assert_info(ch, 301, "wide", False, sp, 16)
    assert ch.info()[3] == 3 and ch.info()[6] == 8
    check(M, ch, sp, refs)


@pytest.mark.parametrize("kind,ncols", [("uniform", [4, 4, 4]), ("wide", [4, 65, 200])])
@pytest.mark.parametrize("name", ["n17", "n1"])
def test_last_wave_of_one_vertex_and_single_vertex_graph(M, name, kind, ncols):
    off, idx = csr(name)
    n = len(off) - 1
    assert off[n] == off[n - 1] and n % 16 == 1   # the last vertex is isolated, alone in its wave
    sp = specs(ncols, 1e-8, [5, 6, 7])
    refs = [oracle(name, s, 30, 0) for s in sp]
    ch = batch(M, device_graph(M, name), kind, sp, 30)   # Graph.from_csr takes the empty edge list of "n1"
    assert_info(ch, n, kind, False, sp, 16)
    check(M, ch, sp, refs)


def test_a_graph_closed_before_its_batch_leaves_no_error_behind(M):
    """A collector finalises the graph and the batch of a failed test in any order. mcmc_chains_destroy used to
    read the device ordinal through the freed graph; the failed hipSetDevice then surfaced as "invalid device
    ordinal" at the error check of the next kernel launch, in another test."""
    sp = uniform(16, 1e-8, 3, 2)
    g = device_graph(M, "rnd")
    ch = batch(M, g, "uniform", sp, 250)
    g.close()
    ch.close()
    ch = batch(M, device_graph(M, "rnd"), "uniform", sp, 250)
    assert_info(ch, 301, "uniform", False, sp, 16)
    check(M, ch, sp, [oracle("rnd", s, 250, 0) for s in sp])


# ---- 5. the tiled drain's second directory round -----------------------------------------------------------------
# 65 column blocks of 65536 ids: no smaller n reaches b0 = 64. The one larger case: the graph's CSR download, the
# one-lane-per-chain init kernel over 4.2e6 vertices, 0.6 GB of colour buffers, two oracle runs on 16 threads.
# Measured on an MI355X: 1.1 s for the graph and its CSR (once), then 1.0 s per batch, oracle included.
N65, P65, SPLIT = 64 * 65536 + 4096, 5e-7, 64 * 65536


@pytest.fixture(scope="module")
def graph65(M):
    g = M.Graph.er_fast(N65, P65, 1)
    s = g.getStruct()

    @lru_cache(maxsize=None)   # the 4-colour chain of seed 4 is in both batches
    def run(spec):
        O.srand(S)
        return O.mcmc_run(s.cumulDegs, s.neighs, spec[0], spec[2], epsilon=spec[1], maxRip=250, sweep_limit=2, nthreads=16)

    yield g, s.cumulDegs, s.neighs, run
    g.close()


@pytest.mark.parametrize("kind,ncols", [("uniform", [4, 4]), ("wide", [65, 4])])
def test_second_directory_round(M, graph65, kind, ncols):
    g, off, idx, run = graph65
    t0 = time.perf_counter()
    lo = off[:-1].astype(np.int64).clip(max=len(idx) - 1)
    has = np.diff(off) > 0
    rowmax, rowmin = np.maximum.reduceat(idx, lo)[has], np.minimum.reduceat(idx, lo)[has]
    assert idx.max() >= SPLIT                          # a neighbour in block 64
    assert ((rowmin < SPLIT) & (rowmax >= SPLIT)).any()   # a row with ids in both rounds
    assert (rowmax < SPLIT).any()                      # a row whose second round is empty
    sp = specs(ncols, 1e-8, [3, 4])
    refs = [run(s) for s in sp]
    ch = batch(M, g, kind, sp, 250)
    assert_info(ch, N65, kind, True, sp, 64)
    check(M, ch, sp, refs, max_sweeps=2)
    print(f"second directory round, {kind}: {time.perf_counter() - t0:.2f} s")
