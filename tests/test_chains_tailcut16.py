"""The batched tail cut of half-word chain batches (csrc/chains_tailcut16.h, mcmc_chains_enable_repair16): chain
r of a repaired batch equals the oracle's run with tailcutRepair and ITS OWN (nCol_r, eps_r, seed_r), exactly --
compare() of test_chains_tailcut.py. Graphs, seeds and maxRip were found with the oracle alone on the CPU; what
each case must show is asserted on the oracle's results."""
import re
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import oracle_ref as O
import tailcut_ref as T
import test_chains_wide16 as W16
from test_chains_tailcut import M, PASSES, compare  # noqa: F401  (M: the module fixture)
from test_chains_wide import S, er_graph, specs

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def csr(name):
    O.srand(1)
    if name == "half":   # degree ~320 > 256: five 64-neighbour chunks per row, split over the repair's four waves
        return O.setup_rnd2(640, 0.5)
    if name == "big":    # degree ~1200 = 4 x 300: a row's neighbours hold colours 0..255 of a 300-colour chain
        return O.setup_rnd2(2400, 0.5)
    return W16.csr(name)


@lru_cache(maxsize=None)
def oracle(name, spec, maxRip, taboo, tailcut, repair=True):
    O.srand(S)
    return O.mcmc_run(*csr(name), spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                      tailcut=tailcut, tailcutRepair=repair)


def batch(M, name, sp, maxRip, taboo, tailcut, passes=PASSES):
    g = er_graph(300, 0.1)[0] if name == "er" else M.Graph.from_csr(*csr(name))
    params = M.ColoringMCMCParams(nCol=0, maxRip=maxRip, tabooIteration=taboo, tailcut=tailcut)
    return M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide16=True, repair16=passes)


def taken(name, s, ref, maxRip, taboo, tailcut):
    """Positions in the chain's colour order of the colours the repair gave, and those colours."""
    before = oracle(name, s, maxRip, taboo, tailcut, False).colors
    new = ref.colors[ref.colors != before]
    order = T.sorted_color_idx(before, s[0]) if tailcut else np.arange(s[0])
    return np.argsort(order)[new], new


EDGE = [40, 257, 288, 511, 512, 513, 1024, 1025, 2047, 2048]
HALF = specs(EDGE, 1e-8, range(3, 13))
G2 = specs([257 + r % 71 for r in range(70)], 1e-8, [3 + 2 * r for r in range(70)])
QUIET = specs([600 + r for r in range(64)] + [16, 16], 1e-8, list(range(3, 67)) + [3, 4])
# graph, (nCol, eps, seed) per chain, maxRip, taboo, tailcut, table words, what the oracle's runs must show
CASES = [
    # the table's word boundaries mixed over the lanes, one chain of 40 colours (a fixed point: it reports the cap);
    # without tailcut the identity order (no table), with it the sorted order with ties
    ("half", HALF[:5], 1, 0, False, 16, "words"), ("half", HALF[:5], 1, 0, True, 16, "ties"),
    ("half", HALF[:7], 1, 0, False, 32, "words"), ("half", HALF[:7], 1, 0, True, 32, "ties"),
    ("half", HALF, 1, 0, False, 64, "words"), ("half", HALF, 1, 0, True, 64, "ties"),
    # identity order: colours 0..255 all held around a flagged vertex, the first free one in a word >= 8
    ("big", specs([300], 1e-8, [3]), 3, 0, False, 16, "word8"),
    ("big", specs([300, 280], 1e-8, [3, 4]), 3, 0, True, 16, "word8"),
    # the tiled instantiations; chains stop at iter = 0 (the flags of C_0) and at iter >= 2 (flag parity)
    ("er", specs([16, 257, 300], 1e-8, [3, 90, 4]), 250, 0, True, 16, "parity"),
    ("er", specs([16, 700, 2048], 1e-8, [3, 5, 6]), 250, 0, True, 64, "parity"),
    ("half", G2, 1, 2, True, 16, None),          # two groups, the second partial (6 chains), taboo
    ("rnd", QUIET, 3, 0, False, 32, "quiet"),    # a group in which no chain needs repair next to one that does
    ("n65", specs([257, 40, 20], 1e-8, [5, 6, 8]), 0, 0, False, 16, "grid"),   # two sweep workgroups with FLAGS
]


@pytest.mark.parametrize("name,sp,maxRip,taboo,tailcut,mw,expect", CASES)
def test_repaired_half_word_chains_match_their_own_oracle(M, name, sp, maxRip, taboo, tailcut, mw, expect):
    refs = [oracle(name, s, maxRip, taboo, tailcut) for s in sp]
    passes = [r.res.tailcutPasses for r in refs]
    assert any(r.traj[-1] > 0 and p >= 1 and r.res.finalViol == 0 for r, p in zip(refs, passes))
    if expect in ("words", "ties", "word8"):
        got = [taken(name, s, r, maxRip, taboo, tailcut) for s, r in zip(sp, refs)]
        assert any(2 <= p < PASSES for p in passes), passes
        assert any(len(pos) and pos.max() >= 32 for pos, _ in got)   # a row that fills the order's first word
        if expect != "words":
            assert any(len(new) and new.max() >= 256 for _, new in got)
        if expect == "word8" and not tailcut:
            assert any(len(pos) and pos.max() >= 256 for pos, _ in got)
    if expect == "ties":
        exits = [oracle(name, s, maxRip, taboo, tailcut, False).colors for s in sp]
        assert any(len(set(np.bincount(c, minlength=s[0]).tolist())) < s[0] for c, s in zip(exits, sp))
    if expect in ("words", "ties"):
        assert passes[0] == PASSES and refs[0].res.finalViol > 0   # 40 colours: the cap through the fixed point
    if expect == "parity":
        assert any(r.res.iter == 0 and r.traj[-1] > 0 for r in refs) and any(r.res.iter >= 2 for r in refs)
    if expect == "quiet":
        assert not any(passes[:64]) and all(passes[64:])
    ch = batch(M, name, sp, maxRip, taboo, tailcut)
    assert ch.info()[0] == (1 if name == "er" else 0) and ch.info()[6] == mw
    if expect == "grid":
        assert ch.info()[4] == 2
    compare(ch, refs)
    assert ch.info()[7] > 0


@pytest.mark.parametrize("cap", [1, 2])
def test_pass_caps_match_the_restatement(M, cap):
    sp = HALF[:6]   # 40 colours: a fixed point that reports the cap; 511 and 513 colours need two passes
    refs = [T.capped_run(*csr("half"), s, 1, 0, False, cap, S) for s in sp]
    assert [r.res.tailcutPasses for r in refs] == [cap, 1, 1, cap, 1, cap]
    assert (refs[3].res.finalViol > 0) == (cap == 1)
    compare(batch(M, "half", sp, 1, 0, False, cap), refs)


def test_errors_and_a_cut_run_repairs_nothing(M):
    from mcmc_colorer_amd._lib import MCMCError, check, lib

    g = M.Graph.from_csr(*csr("half"))
    for kw in ({}, {"wide": True}):   # the narrow and the wide byte batch
        with pytest.raises(MCMCError, match=r"error -1: chains:"):
            M.ColoringMCMCChains(g, M.ColoringMCMCParams(nCol=40), 3, 2, repair16=5, **kw)
    sp = HALF[:5]
    refs = [oracle("half", s, 1, 0, False) for s in sp]
    assert all(r.res.iter == 2 for r in refs)
    ch = batch(M, "half", sp, 1, 0, False)
    assert [(s.tailcutPasses, s.iter) for s in ch.run(1)] == [(0, 1)] * len(sp)
    with pytest.raises(MCMCError, match=r"error -1: chains:"):
        check(lib().mcmc_chains_enable_repair16(ch._h, 5))
    compare(ch, refs)   # the continuing run repairs


def test_cli_default_ncol_chains_with_repair_write_the_repetitions_colour_files(hip_lib, tmp_path):
    from mcmc_colorer_amd._lib import LIB_PATH

    cli = Path(LIB_PATH).parent / "mcmc_colorer"
    common = [str(cli), "--simulate", "0.5", "-n", "640", "--mcmcgpu", "--tailcut", "--tailcutRepair"]   # nCol = maxDeg
    subprocess.run(common + ["--seed", "5", "--chains", "3", "--outDir", str(tmp_path / "b")], check=True,
                   capture_output=True)
    for i in range(3):
        log = subprocess.run(common + ["--seed", str(5 + i), "--repet", "1", "--outDir", str(tmp_path / f"s{i}")],
                             check=True, capture_output=True, text=True).stdout
        assert int(re.search(r"Max Degree: (\d+)", log).group(1)) > 256
        (batch_file,) = (tmp_path / "b").glob(f"*-MCMC_GPU-{i}-colors.txt")
        (single,) = (tmp_path / f"s{i}").glob("*-MCMC_GPU-0-colors.txt")
        assert batch_file.read_text() == single.read_text(), i
