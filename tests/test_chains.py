"""Batched independent chains (csrc/chains.hip) against the oracle: chain r of a batch equals
ColoringMCMC_CPU(g, params, seed + r).run() started at the batch's glibc window -- colouring, full
trajectory, iter, maxIterReached, glibcDraws and initDraws, exactly."""
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import oracle_ref as O

pytestmark = pytest.mark.gpu

S = 1   # srand() seed of every chain's glibc window


@pytest.fixture(scope="module")
def M(hip_lib):
    import mcmc_colorer_amd.colorer as M

    return M


@lru_cache(maxsize=None)
def graph(name):
    O.srand(1)
    if name == "rnd":      # n = 301: 18 full blocks of 16 vertices and one of 13
        return O.setup_rnd2(301, 0.1)
    if name == "dense":    # every degree > 64: every drain takes several 64-neighbour chunks
        return O.setup_rnd2(300, 0.3)
    # "hub": G(230, 0.06) plus vertex 230 adjacent to vertices 0..99 (degree 100 > 64) and the isolated vertex 231
    off, idx = O.setup_rnd2(230, 0.06)
    rows = [list(idx[off[v]:off[v + 1]]) for v in range(230)]
    for v in range(100):
        rows[v].append(230)
    rows += [list(range(100)), []]
    return (np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64), np.array(sum(rows, []), dtype=np.uint32))


@lru_cache(maxsize=None)
def oracle(name, ncol, seed, R, eps, maxRip, taboo, tailcut, sweep_limit):
    off, idx = graph(name)
    out = []
    for r in range(R):
        O.srand(S)
        out.append(O.mcmc_run(off, idx, ncol, seed + r, epsilon=eps, maxRip=maxRip, tabooIteration=taboo,
                              tailcut=tailcut, sweep_limit=sweep_limit))
    return out


# name, nCol, seed, R, eps, maxRip, taboo, tailcut, max_sweeps, what the oracle's runs must show
CASES = [
    ("rnd", 2, 7, 5, 1e-8, 20, 0, False, 0, "cap"),         # no chain converges: maxRip ends every run
    ("rnd", 16, 3, 70, 1e-8, 250, 2, False, 0, "spread"),   # two groups, taboo; chains stop at different sweeps
    ("hub", 33, 11, 64, 1e-8, 250, 0, False, 0, "spread"),  # a full group; degree 100 and degree 0
    ("hub", 16, 5, 5, 1e-8, 250, 2, False, 0, None),
    ("rnd", 64, 2, 1, 1e-8, 250, 0, True, 0, None),         # tail cut: z = 50, the stopping sweep is discarded
    ("rnd", 64, 2, 5, 1e-8, 250, 0, False, 0, "spread"),
    ("rnd", 16, 3, 5, 1e-8, 250, 0, False, 3, None),        # max_sweeps
    # CDF overflows at their natural rate (found by a CPU search with the oracle alone)
    ("dense", 64, 5730, 6, 1e-3, 60, 0, False, 0, "draws"),
    # the ordered replay under load: with eps = 3.3e6 most vertices of colour 0 overflow, every sweep
    ("rnd", 16, 100, 5, 3.3e6, 6, 2, False, 0, "many"),
]


@pytest.mark.parametrize("name,ncol,seed,R,eps,maxRip,taboo,tailcut,max_sweeps,expect", CASES)
def test_chains_match_oracle(M, name, ncol, seed, R, eps, maxRip, taboo, tailcut, max_sweeps, expect):
    refs = oracle(name, ncol, seed, R, eps, maxRip, taboo, tailcut, max_sweeps)
    iters = [r.res.iter for r in refs]
    if expect == "cap":
        assert all(r.res.maxIterReached for r in refs)
    if expect == "spread":
        assert len({r.res.iter for r in refs if not r.res.maxIterReached}) > 1, iters
    if expect == "draws":
        assert sum(r.res.glibcDraws > 0 for r in refs) >= 2, [r.res.glibcDraws for r in refs]
    if expect == "many":
        assert all(r.res.glibcDraws > r.res.iter for r in refs)   # some sweep serves several events of a chain
    off, idx = graph(name)
    g = M.Graph.from_csr(off, idx)
    params = M.ColoringMCMCParams(nCol=ncol, epsilon=eps, maxRip=maxRip, tabooIteration=taboo, tailcut=tailcut)
    ch = M.ColoringMCMCChains(g, params, seed, R, glibc=M.GlibcRand(S, 0))
    stats, cols, trajs = ch.run(max_sweeps), ch.colorings(), ch.trajectories()
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        want = ref.traj[:max_sweeps] if max_sweeps else ref.traj
        assert trajs[r].tolist() == want.tolist(), f"chain {r}"
        assert (st.iter, st.glibcDraws, st.initDraws) == (ref.res.iter, ref.res.glibcDraws, ref.res.initDraws), r
        if not max_sweeps:
            assert (bool(st.maxIterReached), st.finalViol) == (bool(ref.res.maxIterReached), ref.res.finalViol), r
        assert np.array_equal(ch.glibc[r].window, M.GlibcRand(S, ref.res.glibcDraws).window), r


def test_unsupported_ranges_are_argument_errors(M):
    from mcmc_colorer_amd._lib import MCMCError

    g = M.Graph.from_csr(*graph("rnd"))
    for kw, R in (({"nCol": 65}, 4), ({"nCol": 1}, 4), ({"nCol": 16}, 0), ({"nCol": 16}, 1025),
                  ({"nCol": 16, "tailcutRepair": 10}, 4)):
        with pytest.raises(MCMCError, match=r"error -1: chains"):
            M.ColoringMCMCChains(g, M.ColoringMCMCParams(**kw), 1, R)


def test_cli_chains_write_the_repetitions_colour_files(hip_lib, tmp_path):
    from mcmc_colorer_amd._lib import LIB_PATH

    cli = Path(LIB_PATH).parent / "mcmc_colorer"
    common = [str(cli), "--simulate", "0.1", "-n", "300", "--mcmcgpu", "--nCol", "40"]
    subprocess.run(common + ["--seed", "5", "--chains", "3", "--outDir", str(tmp_path / "b")], check=True,
                   capture_output=True)
    for i in range(3):
        subprocess.run(common + ["--seed", str(5 + i), "--repet", "1", "--outDir", str(tmp_path / f"s{i}")],
                       check=True, capture_output=True)
        (batch,) = (tmp_path / "b").glob(f"*-MCMC_GPU-{i}-colors.txt")
        (single,) = (tmp_path / f"s{i}").glob("*-MCMC_GPU-0-colors.txt")
        assert batch.read_text() == single.read_text(), i
