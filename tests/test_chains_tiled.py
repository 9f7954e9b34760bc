"""Batched chains on a generated graph (csrc/chains.hip, the tiled drain): the sweep reads the tiled
16-bit layout, no CSR is built, and chain r equals the oracle's run on the CSR the graph downloads to."""
import ctypes
from functools import lru_cache

import numpy as np
import oracle_ref as O
import pytest

pytestmark = pytest.mark.gpu
S, GSEED = 1, 1   # srand() seed of every chain's glibc window; er_fast seed of every graph


@lru_cache(maxsize=None)
def graph(n, p):
    import mcmc_colorer_amd.colorer as M

    g = M.Graph.er_fast(n, p, GSEED)
    s = g.getStruct()
    return g, s.cumulDegs, s.neighs


@lru_cache(maxsize=None)
def oracle(n, p, ncol, seed, R, eps, maxRip, taboo, sweep_limit):
    _, off, idx = graph(n, p)

    def run(r):
        O.srand(S)
        return O.mcmc_run(off, idx, ncol, seed + r, epsilon=eps, maxRip=maxRip, tabooIteration=taboo, sweep_limit=sweep_limit)

    return [run(r) for r in range(R)]


# n, p, nCol, seed, R, eps, maxRip, taboo, max_sweeps, what the graph / the oracle's runs must show
CASES = [
    (300, 0.1, 16, 3, 70, 1e-8, 250, 2, 0, None),        # one block; layout groups of 32 rows, the last partial; two chain groups
    (300, 0.5, 64, 2, 5, 1e-8, 250, 0, 0, None),         # degree ~150: several chunks per segment, whole rows read
    (300, 0.005, 2, 7, 5, 1e-8, 20, 0, 0, None),         # mostly degree 0 and 1: empty rows, segments of one id and seven pads
    (70000, 3e-4, 16, 4, 3, 1e-8, 250, 0, 4, "blocks"),  # two blocks, short segments packed into one chunk
    (70000, 2e-3, 4, 6, 3, 1e-8, 250, 0, 4, "blocks"),   # degree ~140, 4 colours: the exit fires before block 1
    (300, 0.3, 64, 5, 6, 1e-3, 60, 0, 0, "draws"),       # CDF overflows at their natural rate: records, ordered replay
]


@pytest.mark.parametrize("n,p,ncol,seed,R,eps,maxRip,taboo,max_sweeps,expect", CASES)
def test_tiled_chains_match_oracle(n, p, ncol, seed, R, eps, maxRip, taboo, max_sweeps, expect):
    import mcmc_colorer_amd.colorer as M
    from mcmc_colorer_amd._lib import MCMCError, check, lib

    g, off, idx = graph(n, p)
    refs = oracle(n, p, ncol, seed, R, eps, maxRip, taboo, max_sweeps)
    if expect == "blocks":
        assert idx.max() >= 65536
        rowmax = np.maximum.reduceat(idx, off[:-1].astype(np.int64).clip(max=len(idx) - 1))
        assert (rowmax[np.diff(off) > 0] < 65536).any()   # a row whose block-1 segment is empty
    if expect == "draws":
        assert any(r.res.glibcDraws > 0 for r in refs), [r.res.glibcDraws for r in refs]
    params = M.ColoringMCMCParams(nCol=ncol, epsilon=eps, maxRip=maxRip, tabooIteration=taboo)
    ch = M.ColoringMCMCChains(g, params, seed, R, glibc=M.GlibcRand(S, 0))
    assert ch.info()[0] == 1   # the sweep reads the tiled layout
    stats, cols, trajs = ch.run(max_sweeps), ch.colorings(), ch.trajectories()
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        want = ref.traj[:max_sweeps] if max_sweeps else ref.traj
        assert trajs[r].tolist() == want.tolist(), f"chain {r}"
        assert (st.iter, st.glibcDraws, st.initDraws) == (ref.res.iter, ref.res.glibcDraws, ref.res.initDraws), r
        if not max_sweeps:
            assert (bool(st.maxIterReached), st.finalViol) == (bool(ref.res.maxIterReached), ref.res.finalViol), r
        assert np.array_equal(ch.glibc[r].window, M.GlibcRand(S, ref.res.glibcDraws).window), r
    with pytest.raises(MCMCError, match="no device CSR"):   # no CSR was built behind the caller's back
        check(lib().mcmc_graph_device_ptrs(g.handle, None, None))


def test_raw_abi_takes_an_unmaterialised_graph_and_rejects_a_row_range(hip_lib):
    import mcmc_colorer_amd.colorer as M
    from mcmc_colorer_amd._lib import MCMCError, check, lib, u64ptr

    prm = M.ColoringMCMCParams(nCol=16).to_c(1)
    g, h = M.Graph.er_fast(300, 0.1, GSEED), ctypes.c_void_p()
    check(lib().mcmc_chains_create(g.handle, ctypes.byref(prm), 3, ctypes.byref(h)))
    info = np.zeros(8, dtype=np.uint64)
    check(lib().mcmc_chains_get_info(h, u64ptr(info)))
    lib().mcmc_chains_destroy(h)
    assert info[0] == 1 and info[1] > 2 * 300 * 64 and info[3] == 1 and info[4] * info[2] * 4 >= 300
    part = M.Graph.er_fast(300, 0.1, GSEED, rows=(0, 128))
    with pytest.raises(MCMCError, match=r"error -1: chains"):
        check(lib().mcmc_chains_create(part.handle, ctypes.byref(prm), 3, ctypes.byref(h)))
