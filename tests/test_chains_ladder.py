"""Chain ladders (csrc/chains.hip, the LADDER instantiations of the sweep, and chains_hist_kernel):
chain r of a ladder equals the oracle's run with ITS OWN (nCol_r, eps_r, seed_r) -- colouring, full
trajectory, iter, maxIterReached, finalViol, glibcDraws, initDraws and the advanced glibc window --
and the device histogram of every chain equals the bincount of its colouring."""
import ctypes
from functools import lru_cache

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


def csr(name):
    return er_graph(300, 0.1)[1:] if name == "er" else graph(name)


@lru_cache(maxsize=None)
def oracle(name, spec, maxRip, taboo, sweep_limit):
    off, idx = csr(name)
    O.srand(S)
    return O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                      sweep_limit=sweep_limit)


def specs(ncols, eps, seeds):
    eps = eps if isinstance(eps, (list, tuple)) else [eps] * len(ncols)
    return tuple(zip(ncols, eps, seeds))


# graph, (nCol, eps, seed) per chain, maxRip, taboo, max_sweeps, what the oracle's runs must show
CASES = [
    # chain 0 runs into the cap, the others stop at different sweeps, in both buffers
    ("rnd", specs([2, 16, 33, 64, 17], [1e-8, 1e-6, 1e-8, 1e-4, 1e-8], [7, 302, 12, 4099, 58]), 250, 0, 0, "parities"),
    # two groups, the second partial (6 chains); every nCol from 8 to 64
    ("rnd", specs([8 + r % 57 for r in range(70)], 1e-8, [3 + 2 * r for r in range(70)]), 250, 2, 0, None),
    # every degree > 64: multi-chunk drains, narrow masks fill in the first chunk, the 64-colour ones late
    ("dense", specs([2, 5, 64, 40, 64, 9], 1e-8, [21, 5, 730, 44, 9, 1000]), 40, 0, 0, None),
    # eps = 3.3e6: overflows every sweep, rand() % (nCol_r - 1) with five moduli
    ("rnd", specs([16, 7, 24, 30, 9], 3.3e6, [100, 3, 77, 100, 3]), 6, 2, 0, "many"),
    ("hub", specs([16, 3, 64, 33, 10, 21], 1e-8, [5, 80, 6, 33, 2, 9]), 250, 2, 3, None),   # max_sweeps: all but one still running
    ("er", specs([16, 4, 64, 33, 25], 1e-8, [3, 90, 4, 17, 8]), 250, 0, 0, "tiled"),      # the tiled ladder instantiation
]


@pytest.mark.parametrize("name,sp,maxRip,taboo,max_sweeps,expect", CASES)
def test_ladder_chains_match_their_own_oracle(M, name, sp, maxRip, taboo, max_sweeps, expect):
    g = er_graph(300, 0.1)[0] if name == "er" else M.Graph.from_csr(*graph(name))
    refs = [oracle(name, s, maxRip, taboo, max_sweeps) for s in sp]
    if expect == "parities":
        stops = [r.res.iter for r in refs[1:]]
        assert refs[0].res.maxIterReached and not any(r.res.maxIterReached for r in refs[1:])
        assert len(set(stops)) >= 2 and {i & 1 for i in stops} == {0, 1}, stops
    if expect == "many":
        assert all(r.res.glibcDraws > r.res.iter for r in refs), [(r.res.glibcDraws, r.res.iter) for r in refs]
    params = M.ColoringMCMCParams(nCol=0, maxRip=maxRip, tabooIteration=taboo)
    ch = M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0))
    assert ch.info()[0] == (1 if expect == "tiled" else 0) and ch.info()[5] == 1
    stats, cols, trajs, hist = ch.run(max_sweeps), ch.colorings(), ch.trajectories(), ch.histograms()
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        want = ref.traj[:max_sweeps] if max_sweeps else ref.traj
        assert trajs[r].tolist() == want.tolist(), f"chain {r}"
        assert (st.iter, st.glibcDraws, st.initDraws) == (ref.res.iter, ref.res.glibcDraws, ref.res.initDraws), r
        if not max_sweeps:
            assert (bool(st.maxIterReached), st.finalViol) == (bool(ref.res.maxIterReached), ref.res.finalViol), r
        assert np.array_equal(ch.glibc[r].window, M.GlibcRand(S, ref.res.glibcDraws).window), r
        assert hist[r].tolist() == np.bincount(ref.colors, minlength=64).tolist(), r
        assert not hist[r, sp[r][0]:].any(), r
    rows = ch.summary()
    assert [(d["nCol"], d["seed"], d["iter"], d["min"], d["max"]) for d in rows] == [
        (s[0], s[2], st.iter, int(h[:s[0]].min()), int(h[:s[0]].max())) for s, st, h in zip(sp, stats, hist)]
    conv = [d for d in rows if not d["maxIterReached"]]
    assert ch.best() == (min(conv, key=lambda d: (d["nCol"], d["std"], d["chain"])) if conv else None)


def test_equal_specs_with_consecutive_seeds_are_the_uniform_batch(M):
    g = M.Graph.from_csr(*graph("rnd"))
    params = M.ColoringMCMCParams(nCol=16, epsilon=1e-6, tabooIteration=2)
    uni = M.ColoringMCMCChains(g, params, 3, 6, glibc=M.GlibcRand(S, 0))
    lad = M.ColoringMCMCChains.ladder(g, params, [(16, 1e-6, 3 + r) for r in range(6)], glibc=M.GlibcRand(S, 0))
    assert (uni.info()[5], lad.info()[5]) == (0, 1)
    su, sl = uni.run(), lad.run()
    assert [(s.iter, s.maxIterReached, s.finalViol, s.glibcDraws, s.initDraws) for s in su] == \
           [(s.iter, s.maxIterReached, s.finalViol, s.glibcDraws, s.initDraws) for s in sl]
    assert np.array_equal(uni.colorings(), lad.colorings())
    assert [t.tolist() for t in uni.trajectories()] == [t.tolist() for t in lad.trajectories()]
    assert np.array_equal(uni.histograms(), lad.histograms())   # the histogram serves both kinds of batch


@pytest.mark.parametrize("spec", [(1, 1, 1e-8, 0), (65, 1, 1e-8, 0), (16, 1, 1e-8, 7)])
def test_create_ladder_rejects_bad_specs(M, spec):
    from mcmc_colorer_amd._lib import MCMCChainSpec, MCMCError, check, lib

    g, h = M.Graph.from_csr(*graph("rnd")), ctypes.c_void_p()
    prm = M.ColoringMCMCParams(nCol=16).to_c(1)
    arr = (MCMCChainSpec * 2)(MCMCChainSpec(16, 1, 1e-8, 0), MCMCChainSpec(*spec))
    with pytest.raises(MCMCError, match=r"error -1: chains: chain 1"):
        check(lib().mcmc_chains_create_ladder(g.handle, ctypes.byref(prm), arr, 2, ctypes.byref(h)))
