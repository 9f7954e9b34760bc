"""Wide chain batches (csrc/chains_wide.h: per-lane nCol up to 256, the occupancy masks in a wave-private
LDS table): chain r equals the oracle's run with ITS OWN (nCol_r, eps_r, seed_r) -- colouring, full
trajectory, iter, maxIterReached, finalViol, glibcDraws, initDraws and the advanced glibc window -- and the
device histogram of every chain equals the 256-bin bincount of its colouring."""
import ctypes
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import oracle_ref as O
from test_chains import S, graph
from test_chains_tiled import graph as er_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip_lib):
    import mcmc_colorer_amd.colorer as M

    return M


@lru_cache(maxsize=None)
def csr(name):
    if name == "er":
        return er_graph(300, 0.1)[1:]
    if name == "fill":   # degree ~360: 65 and 80 colours fill a row's mask, mostly before its last chunk
        O.srand(1)
        return O.setup_rnd2(400, 0.9)
    if name == "iso":    # degree ~1.2: a third of the vertices are isolated and never violate
        O.srand(1)
        return O.setup_rnd2(300, 0.004)
    return graph(name)


@lru_cache(maxsize=None)
def oracle(name, spec, maxRip, taboo, sweep_limit=0):
    off, idx = csr(name)
    O.srand(S)
    return O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                      sweep_limit=sweep_limit)


def specs(ncols, eps, seeds):
    eps = eps if isinstance(eps, (list, tuple)) else [eps] * len(ncols)
    return tuple(zip(ncols, eps, seeds))


def covered(name, ref, ncol, whole):
    """Rows of the oracle's initial colouring whose neighbours -- all of them, or those before the row's
    last chunk of 64 -- show every one of the chain's colours: fr == 0, or a full mask ahead of the end."""
    off, idx = (a.astype(np.int64) for a in csr(name))
    ends = off[1:] if whole else off[:-1] + (np.diff(off) - 1).clip(min=0) // 64 * 64
    return {v for v in range(len(off) - 1) if len(np.unique(ref.init[idx[off[v]:ends[v]]])) == ncol}


def check(M, ch, sp, refs, max_sweeps=0):
    stats, cols, trajs, hist = ch.run(max_sweeps), ch.colorings(), ch.trajectories(), ch.histograms()
    assert hist.shape == (len(sp), 256)
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        assert trajs[r].tolist() == (ref.traj[:max_sweeps] if max_sweeps else ref.traj).tolist(), f"chain {r}"
        assert (st.iter, st.glibcDraws, st.initDraws) == (ref.res.iter, ref.res.glibcDraws, ref.res.initDraws), r
        if not max_sweeps:
            assert (bool(st.maxIterReached), st.finalViol) == (bool(ref.res.maxIterReached), ref.res.finalViol), r
        assert np.array_equal(ch.glibc[r].window, M.GlibcRand(S, ref.res.glibcDraws).window), r
        assert hist[r].tolist() == np.bincount(ref.colors, minlength=256).tolist(), r
    return stats


EPS10 = [1e-8, 1e-6, 1e-4, 3e-8, 1e-7, 1e-5, 2e-8, 1e-3, 5e-7, 1e-8]
# graph, (nCol, eps, seed) per chain, maxRip, taboo, mask words, what the graph / the oracle's runs must show
CASES = [
    # every word boundary of the table in one group, mixed over the lanes
    ("rnd", specs([2, 33, 64, 65, 96, 97, 128, 129, 255, 256], EPS10, [7, 12, 4099, 5, 58, 302, 9, 77, 3, 100]), 30, 0, 8, None),
    ("rnd", specs([2, 33, 64, 65, 96, 97, 128, 127, 100, 31], EPS10, [7, 12, 4099, 5, 58, 302, 9, 77, 3, 100]), 30, 0, 4, None),
    # masks fill: fr == 0 rows for 65 and 80 colours; 128 stays open, so the wave's exit needs the next case. Seed 13
    # of the 80-colour chain was found by a CPU search with the oracle alone (its colouring uses all 80 colours).
    ("fill", specs([65, 80, 128], 1e-8, [21, 13, 730]), 12, 0, 4, "fr0"),
    ("fill", specs([65, 70, 80], [1e-8, 1e-6, 1e-8], [21, 44, 13]), 12, 0, 4, "exit"),
    ("dense", specs([200, 256], 1e-8, [9, 1000]), 12, 0, 8, "open"),   # no mask ever fills: every chunk is drained
    # two groups, the second partial (6 chains), taboo
    ("rnd", specs([60 + r % 71 for r in range(70)], 1e-8, [3 + 2 * r for r in range(70)]), 20, 2, 8, None),
    # eps = 3.3e6: every vertex of colour 0 that does not violate overflows, so the isolated ones do every other
    # sweep; rand() % (nCol_r - 1) with the moduli 99, 199, 255 (seed 78: a CPU search with the oracle alone for
    # a 256-colour start that violates at all)
    ("iso", specs([100, 200, 256], 3.3e6, [100, 3, 78]), 6, 2, 8, "many"),
    ("er", specs([16, 65, 130], 1e-8, [3, 90, 4]), 30, 0, 8, "tiled"),   # the tiled instantiation
]


@pytest.mark.parametrize("name,sp,maxRip,taboo,mw,expect", CASES)
def test_wide_chains_match_their_own_oracle(M, name, sp, maxRip, taboo, mw, expect):
    refs = [oracle(name, s, maxRip, taboo) for s in sp]
    if expect == "fr0":
        assert all(covered(name, ref, s[0], True) for s, ref in zip(sp, refs) if s[0] <= 80)
        assert all(r.res.maxIterReached for r in refs)
    if expect == "exit":   # a row at which every chain's mask is full before the row's last chunk
        assert set.intersection(*[covered(name, ref, s[0], False) for s, ref in zip(sp, refs)])
    if expect == "open":
        assert O.max_deg(csr(name)[0]) < min(s[0] for s in sp)
    if expect == "many":
        assert all(r.res.glibcDraws > r.res.iter for r in refs), [(r.res.glibcDraws, r.res.iter) for r in refs]
    g = er_graph(300, 0.1)[0] if name == "er" else M.Graph.from_csr(*csr(name))
    params = M.ColoringMCMCParams(nCol=0, maxRip=maxRip, tabooIteration=taboo)
    ch = M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide=True)
    assert ch.info()[0] == (1 if expect == "tiled" else 0) and ch.info()[5:7] == [1, mw]
    stats = check(M, ch, sp, refs)
    rows = ch.summary()
    assert [(d["nCol"], d["iter"]) for d in rows] == [(s[0], st.iter) for s, st in zip(sp, stats)]
    conv = [d for d in rows if not d["maxIterReached"]]
    assert ch.best() == (min(conv, key=lambda d: (d["nCol"], d["std"], d["chain"])) if conv else None)


def test_max_sweeps_then_a_second_run_continues(M):
    sp, maxRip = specs([65, 80, 128, 200], 1e-8, [21, 13, 730, 4]), 12   # on "fill" nothing converges: all go on
    ch = M.ColoringMCMCChains.ladder(M.Graph.from_csr(*csr("fill")), M.ColoringMCMCParams(nCol=0, maxRip=maxRip), sp,
                                     glibc=M.GlibcRand(S, 0), wide=True)
    check(M, ch, sp, [oracle("fill", s, maxRip, 0, 3) for s in sp], max_sweeps=3)
    check(M, ch, sp, [oracle("fill", s, maxRip, 0) for s in sp])


def fields(ch):
    st = ch.run()
    return ([(s.iter, s.maxIterReached, s.finalViol, s.glibcDraws, s.initDraws) for s in st], ch.colorings().tolist(),
            [t.tolist() for t in ch.trajectories()], [g.window.tolist() for g in ch.glibc], ch.histograms()[:, :64].tolist())


def test_wide_equals_narrow_and_uniform_equals_ladder(M):
    g = M.Graph.from_csr(*graph("rnd"))
    params = M.ColoringMCMCParams(nCol=40, epsilon=1e-6, maxRip=40, tabooIteration=2)
    sp = specs([2, 16, 33, 64, 17], [1e-8, 1e-6, 1e-8, 1e-4, 1e-8], [7, 302, 12, 4099, 58])
    narrow, wide = (M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide=w) for w in (False, True))
    assert (narrow.info()[6], wide.info()[6]) == (0, 4)
    assert fields(narrow) == fields(wide)
    uni = M.ColoringMCMCChains(g, params, 3, 6, glibc=M.GlibcRand(S, 0), wide=True)
    lad = M.ColoringMCMCChains.ladder(g, params, [(40, 1e-6, 3 + r) for r in range(6)], glibc=M.GlibcRand(S, 0), wide=True)
    assert fields(uni) == fields(lad)


def test_argument_errors(M):
    from mcmc_colorer_amd._lib import MCMCChainSpec, MCMCError, check as ok, lib, u32ptr

    g, h = M.Graph.from_csr(*graph("rnd")), ctypes.c_void_p()
    prm = M.ColoringMCMCParams(nCol=16).to_c(1)
    for bad in (257, 1):
        arr = (MCMCChainSpec * 2)(MCMCChainSpec(100, 1, 1e-8, 0), MCMCChainSpec(bad, 1, 1e-8, 0))
        with pytest.raises(MCMCError, match=r"error -1: chains: chain 1"):
            ok(lib().mcmc_chains_create_wide(g.handle, ctypes.byref(prm), arr, 2, ctypes.byref(h)))
    arr = (MCMCChainSpec * 2)(MCMCChainSpec(100, 1, 1e-8, 0), MCMCChainSpec(16, 1, 1e-8, 0))
    ok(lib().mcmc_chains_create_wide(g.handle, ctypes.byref(prm), arr, 2, ctypes.byref(h)))
    out = np.zeros((2, 256), dtype=np.uint32)
    with pytest.raises(MCMCError, match=r"error -1: chains"):
        ok(lib().mcmc_chains_get_histograms(h, u32ptr(out)))
    with pytest.raises(MCMCError, match=r"error -1: chains"):
        ok(lib().mcmc_chains_get_histograms_n(h, u32ptr(out), 99))
    ok(lib().mcmc_chains_get_histograms_n(h, u32ptr(out), 100))
    lib().mcmc_chains_destroy(h)


def test_cli_wide_chains_write_the_repetitions_colour_files(hip_lib, tmp_path):
    from mcmc_colorer_amd._lib import LIB_PATH

    cli = Path(LIB_PATH).parent / "mcmc_colorer"
    common = [str(cli), "--simulate", "0.1", "-n", "300", "--mcmcgpu", "--nCol", "100"]
    subprocess.run(common + ["--seed", "5", "--chains", "3", "--outDir", str(tmp_path / "b")], check=True,
                   capture_output=True)
    for i in range(3):
        subprocess.run(common + ["--seed", str(5 + i), "--repet", "1", "--outDir", str(tmp_path / f"s{i}")],
                       check=True, capture_output=True)
        (batch,) = (tmp_path / "b").glob(f"*-MCMC_GPU-{i}-colors.txt")
        (single,) = (tmp_path / f"s{i}").glob("*-MCMC_GPU-0-colors.txt")
        assert batch.read_text() == single.read_text(), i
