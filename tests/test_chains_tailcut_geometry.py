"""Launch geometry, pass caps and group masks of the batched tail cut (csrc/chains_tailcut.h, chains_repair in
csrc/chains.hip): the paths the production batches take and the ~300-vertex cases of test_chains_tailcut.py never
reach -- a list of several tiles with an empty one between, tiled rows of several chunks over the four waves of
the repair workgroup, rows over two column blocks, the second directory round, vertices per wave other than 16
in the recount, pass caps below 1000 and the fixed-point rule, chain groups that have nothing to repair beside
groups that do, 16 groups, graphs smaller than a wave.

Every comparison is exact (test_chains_tailcut.compare): repaired colouring, tailcutPasses, finalViol, iter,
maxIterReached, trajectory, glibcDraws, initDraws, the device histogram against the bincount of the reference
colouring, best() against summary(). The reference of a batch capped at 1000 passes is the oracle's run with
tailcutRepair; below 1000 it is tests/tailcut_ref.py, whose inputs come from the oracle and which the CPU test
at the end of this module pins to the oracle at 1000 passes. Seeds, maxRip and epsilons were found by CPU
searches with the oracle alone; what each case must show is asserted on the reference before the device is
touched.

Wall times on an MI355X, references included, are noted at the cases."""
import time
from functools import lru_cache

import numpy as np
import pytest

import oracle_ref as O
import tailcut_ref as T
import test_chains_tailcut as TC
from test_chains_geometry import N65, SPLIT, assert_info, csr as named_csr, host_vb, two_blocks, uniform
from test_chains_geometry import graph65  # noqa: F401  (the module-scoped fixture of the 65-block graph)
from test_chains_tiled import GSEED, graph as er_graph
from test_chains_wide import S, specs

gpu = pytest.mark.gpu
PASSES = TC.PASSES   # the oracle's pass cap


@pytest.fixture(scope="module")
def M(hip_lib):
    import mcmc_colorer_amd.colorer as M

    return M


@lru_cache(maxsize=None)
def cpu_csr(name):
    """The graphs of this module without a device: ("er", n, p) from the generator's CPU restatement."""
    if name == "gap":
        return T.gap_graph()
    if isinstance(name, tuple):
        return O.er_fast(name[1], name[2], GSEED)
    return named_csr(name)


def is_tiled(name):
    return isinstance(name, tuple)   # ("er", n, p): a generated graph


def csr(name, cpu=False):
    """A named CSR. A generated graph's is the one the device downloads, or with `cpu` the generator's CPU
    restatement; every other graph is built on the CPU either way."""
    if is_tiled(name) and not cpu:
        return named_csr(name)
    return cpu_csr(name)


def device_graph(M, name):
    return er_graph(*name[1:])[0] if is_tiled(name) else M.Graph.from_csr(*csr(name))


@lru_cache(maxsize=None)
def _reference(name, spec, maxRip, taboo, tailcut, cap, nthreads, cpu):
    off, idx = csr(name, cpu)
    if cap == PASSES:
        O.srand(S)
        return O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                          tailcut=tailcut, tailcutRepair=True, nthreads=nthreads)
    return T.capped_run(off, idx, spec, maxRip, taboo, tailcut, cap, S, nthreads)


def reference(name, spec, maxRip, taboo, tailcut, cap, nthreads=1, cpu=False):
    """Chain `spec` repaired with at most `cap` passes: the oracle at 1000, the restatement below. `cpu` matters
    for a generated graph only, so one cache entry serves both values on every other graph."""
    return _reference(name, spec, maxRip, taboo, tailcut, cap, nthreads, cpu and is_tiled(name))


@lru_cache(maxsize=None)
def _probe(name, spec, maxRip, taboo, tailcut, cap, nthreads, cpu):
    return T.capped_run(*csr(name, cpu), spec, maxRip, taboo, tailcut, cap, S, nthreads, skip_fixed=cap == PASSES)


def probe(name, spec, maxRip, taboo, tailcut, cap, nthreads=1, cpu=False):
    """The restatement's run with its first flags and per-pass (visited, changed, violators), at any cap."""
    return _probe(name, spec, maxRip, taboo, tailcut, cap, nthreads, cpu and is_tiled(name))


def stop_pass(run, cap):
    """The pass after which the host loop stops repairing a chain: no violator left, a pass >= 2 that changed
    nothing (the fixed point), or the cap. 0: nothing to repair."""
    for k, (_, changed, viol) in enumerate(run.history, 1):
        if viol == 0 or (k >= 2 and changed == 0):
            return k
    return min(cap, len(run.history))


def fixed_point(run):
    """f: the first pass >= 2 that changes nothing while violators remain; None if the run shows none."""
    return next((k for k, (_, changed, viol) in enumerate(run.history, 1) if k >= 2 and changed == 0 and viol > 0), None)


def batch(M, name, kind, sp, maxRip, taboo, tailcut, cap):
    """`name`: a graph of csr(), or a device graph itself."""
    g = name if hasattr(name, "handle") else device_graph(M, name)
    params = M.ColoringMCMCParams(nCol=sp[0][0], epsilon=sp[0][1], maxRip=maxRip, tabooIteration=taboo, tailcut=tailcut)
    if kind == "uniform":
        return M.ColoringMCMCChains(g, params, sp[0][2], len(sp), glibc=M.GlibcRand(S, 0), repair=cap)
    return M.ColoringMCMCChains.ladder(g, params, sp, glibc=M.GlibcRand(S, 0), wide=kind == "wide", repair=cap)


def check(ch, refs):
    stats = TC.compare(ch, refs)
    proper = [d for d in ch.summary() if not d["maxIterReached"] or (d["tailcutPasses"] and not d["finalViol"])]
    assert ch.best() == (min(proper, key=lambda d: (d["nCol"], d["std"], d["chain"])) if proper else None)
    assert ch.info()[7] > 0 or not any(r.res.tailcutPasses > 0 for r in refs)
    return stats


def run_case(M, name, kind, sp, maxRip, taboo, tailcut, cap, vb=16, nthreads=1):
    refs = [reference(name, s, maxRip, taboo, tailcut, cap, nthreads) for s in sp]
    ch = batch(M, name, kind, sp, maxRip, taboo, tailcut, cap)
    assert_info(ch, len(csr(name)[0]) - 1, kind, is_tiled(name), sp, vb)
    return check(ch, refs)


# ---- 1. the list kernel over three tiles, the middle one empty ---------------------------------------------------
# maxRip 3, identity colorIdx. 5, 6 and 8 colours end at a fixed point with violators (capped: 3 passes); 9 to 12
# colours repair in one pass, (9, seed 10) in two; 65 colours and more converge in the loop.
GAP = {
    # two groups, the second of six chains
    "uniform": ("uniform", uniform(9, 1e-8, 3, 70), 3, False, 3),
    "ladder": ("ladder", specs([5, 6, 8, 9, 12, 9, 10], 1e-8, [4, 5, 7, 3, 4, 10, 5]), 3, False, 3),
    "wide": ("wide", specs([5, 8, 65, 130, 256, 9, 200], 1e-8, [4, 7, 3, 4, 5, 10, 3]), 3, False, 3),
    # z = 50 and colorIdx sorted by class size, against the oracle itself: 10 colours repair, 7 and 8 do not
    "cut": ("ladder", specs([10, 8, 7], 1e-8, [5, 4, 4]), 250, True, PASSES),
}


def three_tiles(name, sp, maxRip, tailcut):
    """First-pass flags of every group in the tiles [0, 1024) and [2048, n), none in [1024, 2048); the last tile
    is partial and ends inside a wave."""
    n = len(csr(name)[0]) - 1
    assert (n + 1023) // 1024 == 3 and n % 1024 % 64
    for g0 in range(0, len(sp), 64):
        first = np.zeros(n, dtype=bool)
        for s in sp[g0:g0 + 64]:
            run = probe(name, s, maxRip, 0, tailcut, 1)
            if run.history:   # the chain is repaired
                first |= run.first_flags
        assert first[:1024].any() and first[2048:].any() and not first[1024:2048].any(), g0


@gpu
@pytest.mark.parametrize("case", GAP)
def test_list_of_three_tiles_the_middle_one_empty(M, case):   # 0.03 to 0.13 s; uniform 0.7 s (70 references)
    kind, sp, maxRip, tailcut, cap = GAP[case]
    three_tiles("gap", sp, maxRip, tailcut)
    refs = [reference("gap", s, maxRip, 0, tailcut, cap) for s in sp]
    assert any(r.res.tailcutPasses > 0 and r.res.finalViol == 0 for r in refs)   # a chain repaired within the cap
    if case == "ladder":   # the figures of the first chain, as found
        run = probe("gap", sp[0], maxRip, 0, tailcut, 1)
        ff = np.flatnonzero(run.first_flags)
        assert (run.res.iter, (ff < 1024).sum(), (ff >= 2048).sum()) == (4, 330, 276)
        assert refs[0].res.finalViol == 545 and refs[0].res.tailcutPasses == cap
    if case != "uniform":
        assert any(r.res.finalViol > 0 for r in refs)
    run_case(M, "gap", kind, sp, maxRip, 0, tailcut, cap)


# ---- 2. tiled rows of several chunks over the four waves ---------------------------------------------------------
ER600, ER300 = ("er", 600, 0.9), ("er", 300, 0.5)
# graph, nCol per chain (seed 3, maxRip 4), mask words, cap. Degree up to 560: nine chunks over four waves; up to
# 173: three chunks, wave 3 idle. 256 colours on ER600 and 64, 100 on ER300 repair in one pass, the others do not.
# Last: the recount's early exit can fire on a row of several chunks (with 130 colours and more still being repaired
# no row shows every chain a hit among its first 64 neighbours; with 20 and 24 many do).
CHUNKS = {
    "nine-mw8": (ER600, [256, 200, 130], 8, 3, False),
    "nine-mw4": (ER600, [128, 100, 65], 4, 2, False),
    "nine-exit": (ER600, [256, 24, 20], 8, 2, True),
    "three-mw4": (ER300, [64, 100, 40], 4, 3, True),
    "three-mw8": (ER300, [130, 64, 40], 8, 3, True),
}


def early_exit_rows(name, sp, cap):
    """Rows of more than one chunk at which the recount after pass 2 may leave after the first chunk: among the
    first 64 neighbours, in the downloaded order, every chain that pass 2 still repairs has one of the row's
    own colour."""
    off, idx = (a.astype(np.int64) for a in csr(name))
    active = [s for s in sp if probe(name, s, 4, 0, False, 1).res.finalViol > 0]
    cols = [probe(name, s, 4, 0, False, 2).colors for s in active]
    assert active and cap >= 2
    return [v for v in range(len(off) - 1) if off[v + 1] - off[v] > 64
            and all((c[idx[off[v]:off[v] + 64]] == c[v]).any() for c in cols)]


@gpu
@pytest.mark.parametrize("case", CHUNKS)
def test_tiled_rows_of_several_chunks(M, case):   # 0.01 to 0.22 s
    name, ncols, mw, cap, exits = CHUNKS[case]
    sp = specs(ncols, 1e-8, [3] * len(ncols))
    off = csr(name)[0].astype(np.int64)
    deg = np.diff(off)
    first = np.zeros(len(deg), dtype=bool)
    for s in sp:
        run = probe(name, s, 4, 0, False, 1)
        if run.history:
            first |= run.first_flags
    assert (deg[first] > 64).any() and ((deg[first] > 256).any() or name == ER300)
    assert deg.max() > (512 if name == ER600 else 128)   # nine chunks / three chunks
    assert bool(early_exit_rows(name, sp, cap)) == exits
    refs = [reference(name, s, 4, 0, False, cap) for s in sp]
    assert any(r.res.finalViol > 0 for r in refs) and (case == "nine-mw4" or any(
        r.res.tailcutPasses == 1 and r.res.finalViol == 0 for r in refs))
    ch = batch(M, name, "wide", sp, 4, 0, False, cap)
    assert_info(ch, len(deg), "wide", True, sp, 16)
    assert ch.info()[6] == mw
    check(ch, refs)


# ---- 3. rows over two column blocks; the recount on the host's own vb --------------------------------------------
BIG = ("er", 70000, 3e-4)


def rows_on_both_sides(name, first, split):
    off, idx = csr(name)
    lo = off[:-1].astype(np.int64).clip(max=len(idx) - 1)
    has = np.diff(off.astype(np.int64)) > 0
    return int((first & has & (np.minimum.reduceat(idx, lo) < split) & (np.maximum.reduceat(idx, lo) >= split)).sum())


@gpu
@pytest.mark.parametrize("kind", ["uniform", "wide"])
def test_repair_over_two_column_blocks(M, kind):   # uniform 1.6 s (65 oracle runs on 16 threads), wide 0.9 s
    n = BIG[1]
    # uniform: R = 65, two groups, the second of one chain; vb = 18, so the recount's waves end in mid-block of the
    # layout groups. wide: 8 colours cycle to any cap and run against the restatement with cap 2.
    sp = uniform(16, 1e-8, 4, 65) if kind == "uniform" else specs([16, 65, 130, 8], 1e-8, [4, 4, 4, 4])
    cap = PASSES if kind == "uniform" else 2
    assert two_blocks(*csr(BIG))
    run = probe(BIG, sp[0], 3, 0, False, 1, 16)
    assert run.res.iter == 4 and int(run.first_flags.sum()) == 8730 and run.history[0][2] == 0
    assert rows_on_both_sides(BIG, run.first_flags, 65536) > 0
    vb = host_vb(n, len(sp)) if kind == "uniform" else 16
    assert vb == (18 if kind == "uniform" else 16)
    run_case(M, BIG, kind, sp, 3, 0, False, cap, vb=vb, nthreads=16)


# ---- 4. the second directory round -------------------------------------------------------------------------------
# The 65-block graph of test_chains_geometry.py (its fixture, generated once more for this module). 6 colours,
# maxRip 4, seed 4: iter 5, 2405 violators at loop exit, 7633 first-pass flags, 35 of them on rows with neighbours
# below and at or above id 64 * 65536, repaired in one pass; seed 5 likewise. Found by a CPU search with the
# oracle and the restatement: 4 colours end at a fixed point with ~3000 violators whatever maxRip, 5 colours with
# 42; 6 and 8 colours repair in one pass and maxRip 4 gives the shortest list. 65 colours converge in the loop.
# Measured on an MI355X, oracle runs on 16 threads included: 1.10 s for the graph and its CSR (once), then 1.66 s
# (uniform) and 1.11 s (wide) per batch, against 0.96 and 0.86 s of test_second_directory_round in the same run.
D65_MAXRIP = 4
_runs65 = {}


def oracle65(off, idx, spec, **kw):
    key = (spec, tuple(sorted(kw.items())))
    if key not in _runs65:
        O.srand(S)
        _runs65[key] = O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=D65_MAXRIP, nthreads=16, **kw)
    return _runs65[key]


@gpu
@pytest.mark.parametrize("kind,ncols,seeds", [("uniform", [6, 6], [4, 5]), ("wide", [65, 6], [3, 4])])
def test_repair_in_the_second_directory_round(M, graph65, kind, ncols, seeds):
    g, off, idx, _ = graph65
    t0 = time.perf_counter()
    sp = specs(ncols, 1e-8, seeds)
    refs = [oracle65(off, idx, s, tailcutRepair=True) for s in sp]
    chain = sp[seeds.index(4)]
    ref = refs[seeds.index(4)]
    assert (ref.res.iter, ref.res.tailcutPasses, ref.res.finalViol) == (5, 1, 0)   # repaired, within a few passes
    assert all(r.res.tailcutPasses <= 3 and r.res.finalViol == 0 for r in refs)
    first = T.viol_flags(off, idx, oracle65(off, idx, chain, sweep_limit=ref.res.iter - 1).colors.astype(np.int64))
    lo = off[:-1].astype(np.int64).clip(max=len(idx) - 1)
    both = (np.diff(off.astype(np.int64)) > 0) & (np.minimum.reduceat(idx, lo) < SPLIT) & (np.maximum.reduceat(idx, lo) >= SPLIT)
    assert int(first.sum()) == 7633 and int((first & both).sum()) == 35   # flagged rows with ids in both rounds
    ch = batch(M, g, kind, sp, D65_MAXRIP, 0, False, PASSES)
    assert_info(ch, N65, kind, True, sp, 64)
    check(ch, refs)
    print(f"repair in the second directory round, {kind}: {time.perf_counter() - t0:.2f} s")


# ---- 5. pass caps and the fixed point ----------------------------------------------------------------------------
# maxRip 3, identity colorIdx; per graph: a chain repaired in p* = 2 passes, chains that reach a fixed point at
# pass f (2 and 3; 2 and 5; 3 and 4), a chain repaired in one pass. "rnd" also holds the chain whose pass 1 changes
# nothing (epsilon 0.05: the flags of C_{iter-1} name other vertices than C_iter's violators) and whose pass 2
# does: were pass 1 taken for a fixed point, that chain would stop one pass early.
CAPPED = {
    "rnd": (specs([16, 12, 8, 4, 30], [1e-8, 1e-8, 1e-8, 0.05, 1e-8], [10, 3, 8, 68, 3]), 2, (2, 3)),
    "dense": (specs([36, 30, 5, 64], 1e-8, [5, 3, 9, 1000]), 2, (2, 5)),
    "gap": (specs([9, 5, 5, 9], 1e-8, [10, 4, 11, 3]), 2, (3, 4)),
}
CAPS = [(name, cap) for name, (_, p, fs) in CAPPED.items()
        for cap in sorted({1, 2, 3, p - 1, p} | {f + d for f in fs for d in (-1, 0, 1)})]


@gpu
@pytest.mark.parametrize("name,cap", CAPS)
def test_pass_caps_and_the_fixed_point(M, name, cap):   # 0.01 to 0.10 s
    sp, pstar, fs = CAPPED[name]
    full = [probe(name, s, 3, 0, False, 40) for s in sp]
    assert (full[0].res.tailcutPasses, full[0].res.finalViol) == (pstar, 0)
    assert {fixed_point(r) for r in full} >= set(fs)
    assert any(r.res.tailcutPasses == 1 and r.res.finalViol == 0 for r in full)   # beside the capped chains
    if name == "rnd":
        assert any(r.history[0][1] == 0 and r.history[0][2] > 0 and any(h[1] for h in r.history[1:]) for r in full)
    refs = [reference(name, s, 3, 0, False, cap) for s in sp]
    for s, r, long in zip(sp, refs, full):
        assert r.res.tailcutPasses == min(cap, long.res.tailcutPasses)
        assert r.res.finalViol == long.history[r.res.tailcutPasses - 1][2]
        f = fixed_point(long)
        if f and cap > f:   # past its fixed point: the cap, with the colouring of pass f
            fixed = reference(name, s, 3, 0, False, f)
            assert r.res.tailcutPasses == cap and np.array_equal(r.colors, fixed.colors)
    run_case(M, name, "ladder", sp, 3, 0, False, cap)


# ---- 6. group masks ----------------------------------------------------------------------------------------------
NEEDY, EASY = [12, 14, 16, 5], 60
IDLE16, CAP16 = (9, 15), 8
SIXTEEN = specs([40 if r // 64 in IDLE16 else 3 + r % 6 for r in range(1024)], 1e-8, [3 + r for r in range(1024)])


def idle_group_specs(idle):
    """70 chains on "rnd": group `idle` with 60 colours, which converge in the loop; the other with too few."""
    return specs([EASY if r // 64 == idle else NEEDY[r % 4] for r in range(70)], 1e-8, [3 + r for r in range(70)])


@gpu
@pytest.mark.parametrize("kind,idle", [("ladder", 0), ("wide", 1)])
def test_a_group_with_nothing_to_repair_beside_one_that_repairs(M, kind, idle):   # 0.08 and 0.54 s
    """R = 70 on "rnd": the idle group's workgroups leave all three kernels at once, its list is empty, and the
    host copies the counts and changed words of both groups."""
    sp = idle_group_specs(idle)
    refs = [reference("rnd", s, 12, 0, False, PASSES) for s in sp]
    groups = [refs[:64], refs[64:]]
    assert all(r.res.tailcutPasses == 0 and r.res.finalViol == 0 for r in groups[idle])
    assert any(r.res.tailcutPasses > 0 for r in groups[1 - idle])
    run_case(M, "rnd", kind, sp, 12, 0, False, PASSES)


@gpu
def test_16_groups_some_idle_and_chains_of_a_group_stopping_at_different_passes(M):   # 0.15 s
    idle_groups, cap, sp = IDLE16, CAP16, SIXTEEN
    refs = [reference("small", s, 2, 0, False, cap) for s in sp]
    active = [any(r.res.tailcutPasses > 0 for r in refs[g * 64:g * 64 + 64]) for g in range(16)]
    assert [g for g in range(16) if not active[g]] == list(idle_groups)
    assert any(r.res.tailcutPasses and not r.res.finalViol for r in refs) and any(r.res.finalViol for r in refs)
    # chains of one group leave the mask after pass 1 (repaired), 2 and 3 (fixed points)
    assert max(len({stop_pass(r, cap) for r in refs[g * 64:g * 64 + 64]} - {0}) for g in range(16)) >= 3
    ch = batch(M, "small", "ladder", sp, 2, 0, False, cap)
    assert_info(ch, 40, "ladder", False, sp, 16)
    assert ch.info()[3:5] == [16, 1]
    check(ch, refs)


# ---- 7. degenerate graphs ----------------------------------------------------------------------------------------
DEGENERATE = {"uniform": [2, 2, 2], "wide": [2, 65, 200]}


@gpu
@pytest.mark.parametrize("kind,cap", [("uniform", PASSES), ("wide", 5)])
@pytest.mark.parametrize("name", ["n1", "n17", "small"])
def test_repair_on_graphs_smaller_than_a_wave(M, name, kind, cap):   # under 5 ms each
    ncols = DEGENERATE[kind]
    off = csr(name)[0]
    n = len(off) - 1
    sp = specs(ncols, 1e-8, [5, 6, 7])
    refs = [reference(name, s, 6, 0, False, cap) for s in sp]
    if name == "n1":
        assert all(r.res.tailcutPasses == 0 and r.res.finalViol == 0 for r in refs)
    else:   # two colours never colour these graphs: violators at the cap
        assert n < 64 and refs[0].res.tailcutPasses == cap and refs[0].res.finalViol > 0
    if name == "n17":
        assert off[n] == off[n - 1]   # the isolated last vertex
    run_case(M, name, kind, sp, 6, 0, False, cap)


# ---- 8. vertices per wave in the recount and in the flag words ---------------------------------------------------
@gpu
@pytest.mark.parametrize("vb", [1, 5, 1024])
@pytest.mark.parametrize("case", ["gap", "er600"])
def test_block_sizes_with_repair(M, monkeypatch, case, vb):   # 0.01 to 0.15 s
    if case == "gap":
        name, (kind, sp, maxRip, tailcut, cap) = "gap", GAP["ladder"]
    else:
        name, kind, sp, maxRip, tailcut, cap = ER600, "wide", specs(CHUNKS["nine-mw8"][1], 1e-8, [3] * 3), 4, False, 3
    refs = [reference(name, s, maxRip, 0, tailcut, cap) for s in sp]   # before the device, as every property
    assert any(r.res.tailcutPasses > 1 for r in refs)
    monkeypatch.setenv("MCMC_CHAINS_VB", str(vb))   # read by getenv when the batch is created
    run_case(M, name, kind, sp, maxRip, 0, tailcut, cap, vb=vb)


# ---- the restatement against the oracle (CPU) --------------------------------------------------------------------
def pinned_chains():
    """(graph, spec, maxRip, taboo, tailcut) of every chain of this module on a graph of n <= 3000 and of the
    CASES of test_chains_tailcut.py."""
    out = []
    for kind, sp, maxRip, tailcut, _ in GAP.values():
        out += [("gap", s, maxRip, 0, tailcut) for s in sp]
    for name, ncols, *_ in CHUNKS.values():
        out += [(name, s, 4, 0, False) for s in specs(ncols, 1e-8, [3] * len(ncols))]
    for name, (sp, _, _) in CAPPED.items():
        out += [(name, s, 3, 0, False) for s in sp]
    for idle in (0, 1):
        out += [("rnd", s, 12, 0, False) for s in idle_group_specs(idle)]
    out += [("small", s, 2, 0, False) for s in SIXTEEN]
    for name in ("n1", "n17", "small"):
        out += [(name, s, 6, 0, False) for ncols in DEGENERATE.values() for s in specs(ncols, 1e-8, [5, 6, 7])]
    for name, _, sp, maxRip, taboo, tailcut, _ in TC.CASES:
        out += [(name if name != "er" else ("er", 300, 0.1), s, maxRip, taboo, tailcut) for s in sp]
    return sorted(set(out), key=str)


def test_the_restatement_equals_the_oracle_at_1000_passes():   # 14 s on the CPU: cycling chains run 1000 Python passes
    chains = pinned_chains()
    repaired = ties = 0
    for name, spec, maxRip, taboo, tailcut in chains:
        ref = reference(name, spec, maxRip, taboo, tailcut, PASSES, cpu=True)
        run = probe(name, spec, maxRip, taboo, tailcut, PASSES, cpu=True)
        assert np.array_equal(run.colors, ref.colors), (name, spec)
        assert (run.res.tailcutPasses, run.res.finalViol) == (ref.res.tailcutPasses, ref.res.finalViol), (name, spec)
        assert (run.res.iter, run.traj.tolist()) == (ref.res.iter, ref.traj.tolist()), (name, spec)
        repaired += ref.res.tailcutPasses > 0
        if tailcut and ref.res.tailcutPasses:   # the sorted colorIdx decided, among equal class sizes too
            O.srand(S)
            loop = O.mcmc_run(*csr(name, True), spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                              tailcut=True).colors
            ties += len(set(np.bincount(loop, minlength=spec[0]).tolist())) < spec[0]
    assert repaired > 40 and ties > 3, (repaired, ties)


def test_the_fixed_point_skip_of_the_pin_changes_nothing():
    """The pin above ends a run at a pass that left colouring and flags as it met them; the capped references
    run every pass. Both give the same result on chains that meet a fixed point below the cap."""
    for name, spec in (("dense", (5, 1e-8, 9)), ("gap", (5, 1e-8, 4)), ("rnd", (4, 0.05, 68))):
        plain = T.capped_run(*csr(name), spec, 3, 0, False, 7, S)
        skip = T.capped_run(*csr(name), spec, 3, 0, False, 7, S, skip_fixed=True)
        assert fixed_point(plain) and len(skip.history) <= fixed_point(plain) < 7 == len(plain.history)
        assert np.array_equal(plain.colors, skip.colors)
        assert (plain.res.tailcutPasses, plain.res.finalViol) == (skip.res.tailcutPasses, skip.res.finalViol) == (7, plain.history[-1][2])


def test_std_sort_restatement_is_a_sort_and_keeps_short_ties_in_order():
    rng = np.random.default_rng(1)
    for k in (2, 14, 16, 17, 65, 130, 256):
        keys = rng.integers(0, 12, k).tolist()
        order = T.std_sort_indices(keys)
        assert sorted(order) == list(range(k)) and all(keys[a] <= keys[b] for a, b in zip(order, order[1:]))
        if k <= 16:   # one insertion sort: stable
            assert order == sorted(range(k), key=keys.__getitem__)
