"""The batched tail cut (csrc/chains_tailcut.h, mcmc_chains_enable_repair): chain r of a repaired batch
equals the oracle's run with tailcutRepair and ITS OWN (nCol_r, eps_r, seed_r) -- the repaired colouring,
tailcutPasses, finalViol, iter, maxIterReached, the loop's trajectory, glibcDraws, initDraws -- and the
device histogram equals the bincount of the repaired colouring. Seeds and maxRip were found by a CPU
search with the oracle alone; what each case must show is asserted on the oracle's results."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_ref as O
from test_chains_wide import S, csr, er_graph, specs

pytestmark = pytest.mark.gpu
PASSES = 1000   # the oracle's pass cap


@pytest.fixture(scope="module")
def M(hip_lib):
    import mcmc_colorer_amd.colorer as M

    return M


def oracle(name, spec, maxRip, taboo, tailcut, repair=True, sweep_limit=0):
    off, idx = csr(name)
    O.srand(S)
    return O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo, tailcut=tailcut,
                      tailcutRepair=repair, sweep_limit=sweep_limit)


def flagged_neighbours(name, colors):
    """Per arc (v, w): both ends violate in `colors`."""
    off, idx = (a.astype(np.int64) for a in csr(name))
    src = np.repeat(np.arange(len(off) - 1), np.diff(off))
    viol = np.zeros(len(off) - 1, dtype=bool)
    viol[src[colors[src] == colors[idx]]] = True
    return viol[src] & viol[idx]


def show(name, sp, refs, maxRip, taboo, tailcut, expect):
    loop = [r.traj[-1] for r in refs]   # Cviol at loop exit
    if expect == "cut":   # the loop ran and the cut stopped a chain with violators; its class sizes tie
        exits = [oracle(name, s, maxRip, taboo, tailcut, False).colors for s in sp]
        assert any(r.res.iter >= 1 and 0 < lv <= 50 and len(set(np.bincount(c, minlength=s[0]).tolist())) < s[0]
                   for r, lv, c, s in zip(refs, loop, exits, sp)), loop
    if expect == "gs":    # first-pass flags (those of C_{iter-1}) on both ends of an edge: Gauss-Seidel != Jacobi
        r, s = refs[0], sp[0]
        assert r.res.maxIterReached and loop[0] > 0
        before = oracle(name, s, maxRip, taboo, tailcut, False, r.res.iter - 1).colors
        assert flagged_neighbours(name, before).any()
    if expect == "parity":
        assert {r.res.iter & 1 for r in refs} == {0, 1} and len({r.res.iter for r in refs}) > 2
        assert any(r.res.iter == 0 and lv > 0 for r, lv in zip(refs, loop)), [(r.res.iter, lv) for r, lv in zip(refs, loop)]
    if expect == "cap":
        assert any(r.res.tailcutPasses == PASSES and r.res.finalViol > 0 for r in refs)
        assert any(r.res.tailcutPasses > 0 and r.res.finalViol == 0 for r in refs)
    assert any(r.res.tailcutPasses > 0 for r in refs)


def batch(M, name, kind, sp, maxRip, taboo, tailcut):
    g = er_graph(300, 0.1)[0] if name == "er" else M.Graph.from_csr(*csr(name))
    params = M.ColoringMCMCParams(nCol=sp[0][0], epsilon=sp[0][1], maxRip=maxRip, tabooIteration=taboo, tailcut=tailcut)
    if kind == "uniform":
        return M.ColoringMCMCChains(g, params, sp[0][2], len(sp), glibc=M.GlibcRand(S, 0), repair=PASSES)
    return M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide=kind == "wide", repair=PASSES)


def compare(ch, refs):
    stats, cols, trajs, hist = ch.run(), ch.colorings(), ch.trajectories(), ch.histograms()
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        assert (st.tailcutPasses, st.finalViol) == (ref.res.tailcutPasses, ref.res.finalViol), r
        assert (st.iter, bool(st.maxIterReached)) == (ref.res.iter, bool(ref.res.maxIterReached)), r
        assert trajs[r].tolist() == ref.traj.tolist(), r
        assert (st.glibcDraws, st.initDraws) == (ref.res.glibcDraws, ref.res.initDraws), r
        assert hist[r].tolist() == np.bincount(ref.colors, minlength=hist.shape[1]).tolist(), r
    return stats


CUT = ("rnd", "uniform", specs([14] * 5, 1e-8, range(3, 8)), 250, 0, True, "cut")
# graph, batch kind, (nCol, eps, seed) per chain, maxRip, taboo, tailcut, what the oracle's runs must show
CASES = [
    CUT,                                                                        # z = 50, colorIdx sorted, ties
    ("rnd", "uniform", specs([16] * 5, 1e-8, range(3, 8)), 3, 0, False, "gs"),  # the cap: identity colorIdx, many flags
    # chains stop at different sweeps of both parities in one group, one at iter = 0 with violators: the merged
    # flag words, the parity select, the normalise step
    ("iso", "ladder", specs([2, 2, 3, 3, 2, 3, 8, 8], 1e-8, [7, 12, 5, 58, 302, 9, 77, 3]), 250, 2, True, "parity"),
    # degree ~360: a row spans several chunks per wave, the waves' ORs meet in the LDS table; 8 and 4 mask words
    ("fill", "wide", specs([65, 128, 129, 255, 256], 1e-8, [21, 730, 4, 9, 1000]), 6, 0, False, "gs"),
    ("fill", "wide", specs([65, 100, 128], 1e-8, [21, 13, 730]), 6, 0, True, None),
    ("er", "ladder", specs([14, 15, 16], 1e-8, [3, 90, 4]), 250, 0, True, "cut"),   # the tiled instantiations
    ("er", "wide", specs([16, 65, 130], 1e-8, [3, 90, 4]), 3, 0, False, None),
    ("rnd", "uniform", specs([14] * 70, 1e-8, range(3, 73)), 250, 2, True, None),   # two groups, the second partial
    # 5 colours can never colour G(300, 0.3): the pass cap, reached through the fixed point; 64 colours repair
    ("dense", "ladder", specs([5, 64], 1e-8, [9, 1000]), 3, 0, False, "cap"),
]


@pytest.mark.parametrize("name,kind,sp,maxRip,taboo,tailcut,expect", CASES)
def test_repaired_chains_match_their_own_oracle(M, name, kind, sp, maxRip, taboo, tailcut, expect):
    refs = [oracle(name, s, maxRip, taboo, tailcut) for s in sp]
    show(name, sp, refs, maxRip, taboo, tailcut, expect)
    ch = batch(M, name, kind, sp, maxRip, taboo, tailcut)
    compare(ch, refs)
    proper = [d for d in ch.summary() if not d["maxIterReached"] or (d["tailcutPasses"] and not d["finalViol"])]
    assert ch.best() == (min(proper, key=lambda d: (d["nCol"], d["std"], d["chain"])) if proper else None)
    assert ch.info()[7] > 0


def test_enable_after_a_run_started_is_refused_and_a_cut_run_repairs_nothing(M):
    from mcmc_colorer_amd._lib import MCMCError, check, lib

    name, kind, sp, maxRip, taboo, tailcut, _ = CUT
    refs = [oracle(name, s, maxRip, taboo, tailcut) for s in sp]
    assert all(r.res.iter > 2 for r in refs)
    ch = batch(M, name, kind, sp, maxRip, taboo, tailcut)
    assert [(s.tailcutPasses, s.iter) for s in ch.run(2)] == [(0, 2)] * len(sp)
    with pytest.raises(MCMCError, match=r"error -1: chains"):
        check(lib().mcmc_chains_enable_repair(ch._h, 5))
    compare(ch, refs)   # the continuing run repairs


def test_cli_chains_with_repair_write_the_repetitions_colour_files(hip_lib, tmp_path):
    from mcmc_colorer_amd._lib import LIB_PATH

    cli = Path(LIB_PATH).parent / "mcmc_colorer"
    common = [str(cli), "--simulate", "0.1", "-n", "300", "--mcmcgpu", "--nCol", "14", "--tailcut", "--tailcutRepair"]
    subprocess.run(common + ["--seed", "5", "--chains", "3", "--outDir", str(tmp_path / "b")], check=True,
                   capture_output=True)
    for i in range(3):
        subprocess.run(common + ["--seed", str(5 + i), "--repet", "1", "--outDir", str(tmp_path / f"s{i}")],
                       check=True, capture_output=True)
        (batch_file,) = (tmp_path / "b").glob(f"*-MCMC_GPU-{i}-colors.txt")
        (single,) = (tmp_path / f"s{i}").glob("*-MCMC_GPU-0-colors.txt")
        assert batch_file.read_text() == single.read_text(), i
