"""Half-word chain batches (csrc/chains_wide16.h: per-lane nCol up to 2048, 16-bit colours, the counted OR
into a wave-private LDS table, the run-and-binade CDF walk): chain r equals the oracle's run with ITS OWN
(nCol_r, eps_r, seed_r) -- colouring, full trajectory, iter, maxIterReached, finalViol, glibcDraws,
initDraws and the advanced glibc window -- and the device histogram of every chain equals the bincount of
its colouring. Every comparison is exact equality."""
import ctypes
import re
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import oracle_ref as O
import test_chains_wide as W
from test_chains_wide import M, S, er_graph, fields, specs  # noqa: F401  (M: the module fixture)

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def csr(name):
    if name == "fill16":   # degree ~2160, about 8 x 270: 257 and 270 colours fill a row's table
        O.srand(1)
        return O.setup_rnd2(2400, 0.9)
    if name == "n65":      # the smallest n with two sweep workgroups (4 waves of 16 vertices)
        O.srand(1)
        return O.setup_rnd2(65, 0.3)
    return W.csr(name)


@lru_cache(maxsize=None)
def oracle(name, spec, maxRip, taboo):
    if name not in ("fill16", "n65"):
        return W.oracle(name, spec, maxRip, taboo)
    O.srand(S)
    return O.mcmc_run(*csr(name), spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo)


def check(M, ch, sp, refs):
    stats, cols, trajs, hist = ch.run(), ch.colorings(), ch.trajectories(), ch.histograms()
    width = max(s[0] for s in sp)
    assert hist.shape == (len(sp), width)
    for r, (ref, st) in enumerate(zip(refs, stats)):
        assert np.array_equal(cols[r], ref.colors), f"chain {r}: {np.flatnonzero(cols[r] != ref.colors)[:8]}"
        assert trajs[r].tolist() == ref.traj.tolist(), f"chain {r}"
        assert (st.iter, st.glibcDraws, st.initDraws) == (ref.res.iter, ref.res.glibcDraws, ref.res.initDraws), r
        assert (bool(st.maxIterReached), st.finalViol) == (bool(ref.res.maxIterReached), ref.res.finalViol), r
        assert np.array_equal(ch.glibc[r].window, M.GlibcRand(S, ref.res.glibcDraws).window), r
        assert hist[r].tolist() == np.bincount(ref.colors, minlength=width).tolist(), r
    return stats


EPS = [1e-8, 1e-6, 1e-4, 3e-8, 1e-7, 1e-5, 2e-8, 1e-3, 5e-7, 1e-8, 1e-6, 1e-8, 1e-7]
SEEDS = [7, 12, 4099, 5, 58, 302, 9, 77, 3, 100, 41, 8, 6]
EDGE = [2, 64, 256, 257, 288, 289, 511, 512, 513, 1024, 1025, 2047, 2048]
# graph, (nCol, eps, seed) per chain, maxRip, taboo, table words, what the graph / the oracle's runs must show
CASES = [
    # the table's word-count boundaries in one group, mixed over the lanes
    ("rnd", specs(EDGE[:8], EPS[:8], SEEDS[:8]), 30, 0, 16, None),
    ("rnd", specs(EDGE[:10], EPS[:10], SEEDS[:10]), 30, 0, 32, None),
    ("rnd", specs(EDGE, EPS, SEEDS), 30, 0, 64, None),
    # tables fill: fr == 0 rows for 257 and 270 colours; 600 stays open, so the wave's exit needs the next case
    ("fill16", specs([257, 270, 600], 1e-8, [21, 13, 730]), 3, 0, 32, "fr0"),
    ("fill16", specs([257, 263, 270], [1e-8, 1e-6, 1e-8], [21, 45, 13]), 3, 0, 16, "exit"),
    ("dense", specs([300, 2048], 1e-8, [9, 1000]), 12, 0, 64, "open"),   # no table ever fills: every chunk is drained
    # two groups, the second partial (6 chains), taboo: the group offset in half-word elements
    ("rnd", specs([257 + r % 71 for r in range(70)], 1e-8, [3 + 2 * r for r in range(70)]), 20, 2, 16, None),
    # eps = 3.3e6: every vertex of colour 0 that does not violate overflows, so rand() % (nCol_r - 1) with the
    # moduli 299, 699 and 2047 yields colours >= 256 (seeds: a CPU search with the oracle alone for a start with
    # a vertex of colour 0). At nCol = 1000 the fp32 walk hi + 999 x eps ends at +17888 > u, so that chain cannot
    # overflow from colour 0 (no seed below 6000 draws more than once): it runs and is compared, 700 stands in
    # for it in the draw count.
    ("iso", specs([300, 1000, 2048, 700], 3.3e6, [3, 5, 14, 5]), 6, 2, 64, "many"),
    ("er", specs([16, 257, 700], 1e-8, [3, 90, 4]), 30, 0, 32, "tiled"),   # the tiled instantiation
    ("n65", specs([257, 40], 1e-8, [5, 6]), 30, 0, 16, "grid"),           # more than one sweep workgroup
]


@pytest.mark.parametrize("name,sp,maxRip,taboo,mw,expect", CASES)
def test_wide16_chains_match_their_own_oracle(M, name, sp, maxRip, taboo, mw, expect):
    refs = [oracle(name, s, maxRip, taboo) for s in sp]
    if expect in ("fr0", "exit"):
        off, idx = (a.astype(np.int64) for a in csr(name))
        ends = {True: off[1:], False: off[:-1] + (np.diff(off) - 1).clip(min=0) // 64 * 64}

        def covered(ref, ncol, whole):   # W.covered's rows, on this file's graph
            return {v for v in range(len(off) - 1) if len(np.unique(ref.init[idx[off[v]:ends[whole][v]]])) == ncol}

        if expect == "fr0":
            assert all(covered(ref, s[0], True) for s, ref in zip(sp, refs) if s[0] <= 270)
        else:   # a row at which every chain's table is full before the row's last chunk
            assert set.intersection(*[covered(ref, s[0], False) for s, ref in zip(sp, refs)])
    if expect == "open":
        assert O.max_deg(csr(name)[0]) < min(s[0] for s in sp)
    if expect == "many":
        assert all(r.res.glibcDraws > r.res.iter for s, r in zip(sp, refs) if s[0] != 1000)
    g = er_graph(300, 0.1)[0] if name == "er" else M.Graph.from_csr(*csr(name))
    params = M.ColoringMCMCParams(nCol=0, maxRip=maxRip, tabooIteration=taboo)
    ch = M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide16=True)
    assert ch.info()[0] == (1 if expect == "tiled" else 0) and ch.info()[5:7] == [1, mw]
    if expect == "grid":
        assert ch.info()[4] == 2
    stats = check(M, ch, sp, refs)
    rows = ch.summary()
    assert [(d["nCol"], d["iter"]) for d in rows] == [(s[0], st.iter) for s, st in zip(sp, stats)]
    conv = [d for d in rows if not d["maxIterReached"]]
    assert ch.best() == (min(conv, key=lambda d: (d["nCol"], d["std"], d["chain"])) if conv else None)


def test_argument_errors_and_small_batches_equal_the_narrow_ladder(M):
    from mcmc_colorer_amd._lib import MCMCChainSpec, MCMCError, check as ok, lib, u32ptr

    g, h = M.Graph.from_csr(*csr("rnd")), ctypes.c_void_p()
    prm = M.ColoringMCMCParams(nCol=16).to_c(1)
    for bad in (2049, 1):
        arr = (MCMCChainSpec * 2)(MCMCChainSpec(100, 1, 1e-8, 0), MCMCChainSpec(bad, 1, 1e-8, 0))
        with pytest.raises(MCMCError, match=r"error -1: chains: chain 1"):
            ok(lib().mcmc_chains_create_wide16(g.handle, ctypes.byref(prm), arr, 2, ctypes.byref(h)))
    arr = (MCMCChainSpec * 2)(MCMCChainSpec(300, 1, 1e-8, 0), MCMCChainSpec(16, 1, 1e-8, 0))
    ok(lib().mcmc_chains_create_wide16(g.handle, ctypes.byref(prm), arr, 2, ctypes.byref(h)))
    out = np.zeros((2, 300), dtype=np.uint32)
    for refused in (lambda: lib().mcmc_chains_get_histograms(h, u32ptr(out)),
                    lambda: lib().mcmc_chains_get_histograms_n(h, u32ptr(out), 299),
                    lambda: lib().mcmc_chains_enable_repair(h, 5)):
        with pytest.raises(MCMCError, match=r"error -1: chains"):
            ok(refused())
    ok(lib().mcmc_chains_get_histograms_n(h, u32ptr(out), 300))
    lib().mcmc_chains_destroy(h)
    with pytest.raises(MCMCError, match=r"error -1: chains"):
        M.ColoringMCMCChains(g, M.ColoringMCMCParams(nCol=300), 3, 2, wide16=True, repair=5)
    params = M.ColoringMCMCParams(nCol=40, epsilon=1e-6, maxRip=40, tabooIteration=2)
    sp = specs([2, 16, 33, 64, 17], [1e-8, 1e-6, 1e-8, 1e-4, 1e-8], [7, 302, 12, 4099, 58])
    narrow, half = (M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide16=w) for w in (False, True))
    assert (narrow.info()[6], half.info()[6]) == (0, 16)
    assert fields(narrow) == fields(half)
    uni = M.ColoringMCMCChains(g, params, 3, 6, glibc=M.GlibcRand(S, 0), wide16=True)
    lad = M.ColoringMCMCChains.ladder(g, params, [(40, 1e-6, 3 + r) for r in range(6)], glibc=M.GlibcRand(S, 0), wide16=True)
    assert fields(uni) == fields(lad)


def test_cli_default_ncol_chains_write_the_repetitions_colour_files(hip_lib, tmp_path):
    from mcmc_colorer_amd._lib import LIB_PATH

    cli = Path(LIB_PATH).parent / "mcmc_colorer"
    common = [str(cli), "--simulate", "0.3", "-n", "1000", "--mcmcgpu"]   # no --nCol: the reference's default, maxDeg
    subprocess.run(common + ["--seed", "5", "--chains", "3", "--outDir", str(tmp_path / "b")], check=True,
                   capture_output=True)
    for i in range(3):
        log = subprocess.run(common + ["--seed", str(5 + i), "--repet", "1", "--outDir", str(tmp_path / f"s{i}")],
                             check=True, capture_output=True, text=True).stdout
        assert int(re.search(r"Max Degree: (\d+)", log).group(1)) > 256
        (batch,) = (tmp_path / "b").glob(f"*-MCMC_GPU-{i}-colors.txt")
        (single,) = (tmp_path / f"s{i}").glob("*-MCMC_GPU-0-colors.txt")
        assert batch.read_text() == single.read_text(), i
