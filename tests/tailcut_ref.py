"""A plain restatement of the corrected tail cut (oracle/mcmc_cpu_ref.cpp::tail_cut) with a pass cap of the
caller's choice -- TEST INFRASTRUCTURE ONLY. The oracle's cap is fixed at 1000; the batched repair
(mcmc_chains_enable_repair) takes any. tests/test_chains_tailcut_geometry.py pins this restatement to the
oracle at 1000 passes and compares the device with it below that.

No shortcut of the device's host loop is used for a capped reference: a chain at a fixed point simply runs its
passes."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import oracle_ref as O


def viol_flags(off, idx, colors) -> np.ndarray:
    """Per vertex: some neighbour holds its colour."""
    off = off.astype(np.int64)
    deg = np.diff(off)
    if not len(idx):
        return np.zeros(len(deg), dtype=bool)
    same = colors[idx] == np.repeat(colors, deg)
    return np.logical_or.reduceat(same, off[:-1].clip(max=len(idx) - 1)) & (deg > 0)


def tail_cut_ref(off, idx, colors_at_loop_exit, first_flags, colorIdx, max_passes, history=None, skip_fixed=False):
    """(colors, passes, finalViol) after at most max_passes passes. A pass visits the flagged vertices in ascending
    order; each takes the first colour of colorIdx that no neighbour holds, reading what the pass has already
    written, and stays as it is when none is free; then the flags and their count are recomputed in full. The
    first pass visits first_flags; passes run while violators remain. `history` (a list) receives, per pass,
    (vertices visited, vertices whose colour changed, violators after the pass). skip_fixed: a pass that leaves
    both the colouring and the flags as it met them ends the run at max_passes (only the comparison with the
    oracle's 1000 passes uses it, to stay quick; the oracle runs them all)."""
    off = off.astype(np.int64)
    C = np.array(colors_at_loop_exit, dtype=np.int64)
    order = [int(c) for c in colorIdx]
    viol = int(viol_flags(off, idx, C).sum())
    flags = np.asarray(first_flags, dtype=bool)
    passes = 0
    while viol > 0 and passes < max_passes:
        visited = np.flatnonzero(flags).tolist()
        changed = 0
        for v in visited:
            held = set(C[idx[off[v]:off[v + 1]]].tolist())
            for c in order:
                if c not in held:
                    changed += int(C[v] != c)
                    C[v] = c
                    break
        before, flags = flags, viol_flags(off, idx, C)
        viol = int(flags.sum())
        passes += 1
        if history is not None:
            history.append((len(visited), changed, viol))
        if skip_fixed and viol > 0 and changed == 0 and np.array_equal(before, flags):
            passes = max_passes   # the same flags over the same colouring: every further pass is this one
    return C.astype(np.uint32), passes, viol


def std_sort_indices(keys) -> list:
    """std::sort(colorIdx, [&](int i, int j) { return keys[i] < keys[j]; }) over the identity, as libstdc++ runs
    it (introsort: median-of-three partitions above 16 elements, then insertion sorts): equal keys end in the
    library's order, which the reference's colorIdx inherits. The heap-sort fallback of a degenerate partition
    depth is not restated; it is refused."""
    a = list(range(len(keys)))

    def less(i, j):
        return keys[i] < keys[j]

    def swap(i, j):
        a[i], a[j] = a[j], a[i]

    def median_to_first(res, x, y, z):
        if less(a[x], a[y]):
            swap(res, y if less(a[y], a[z]) else z if less(a[x], a[z]) else x)
        else:
            swap(res, x if less(a[x], a[z]) else z if less(a[y], a[z]) else y)

    def partition(first, last, pivot):
        while True:
            while less(a[first], a[pivot]):
                first += 1
            last -= 1
            while less(a[pivot], a[last]):
                last -= 1
            if not first < last:
                return first
            swap(first, last)
            first += 1

    def loop(first, last, depth):
        while last - first > 16:
            assert depth > 0, "heap-sort fallback"
            depth -= 1
            median_to_first(first, first + 1, first + (last - first) // 2, last - 1)
            cut = partition(first + 1, last, first)
            loop(cut, last, depth)
            last = cut

    def insert(i, guarded):
        val = a[i]
        if guarded and less(val, a[0]):
            a[1:i + 1] = a[0:i]
            a[0] = val
            return
        while less(val, a[i - 1]):
            a[i] = a[i - 1]
            i -= 1
        a[i] = val

    n = len(a)
    if n > 1:
        loop(0, n, 2 * (n.bit_length() - 1))
        for i in range(1, n):
            insert(i, i < 16)
    return a


def sorted_color_idx(colors, ncol) -> np.ndarray:
    """colorIdx of a cut run (z > 0): the colours by ascending class size, ties as std::sort leaves them."""
    return np.asarray(std_sort_indices(np.bincount(colors, minlength=ncol).tolist()))


@dataclass
class CappedRun:
    """What compare() of test_chains_tailcut.py reads of an oracle run, from the restatement."""
    colors: np.ndarray
    traj: np.ndarray
    res: object
    history: list
    first_flags: np.ndarray


@dataclass
class CappedResult:
    iter: int
    maxIterReached: int
    finalViol: int
    glibcDraws: int
    initDraws: int
    tailcutPasses: int


def capped_run(off, idx, spec, maxRip, taboo, tailcut, cap, S=1, nthreads=1, skip_fixed=False) -> CappedRun:
    """Chain `spec` = (nCol, eps, seed) with at most `cap` repair passes. Every input of the restatement comes
    from the oracle: the loop-exit colouring from its run without repair, the first flags from C_{iter-1} (its
    run stopped one sweep earlier; the initial colouring when iter <= 1)."""
    def run(**kw):
        O.srand(S)
        return O.mcmc_run(off, idx, spec[0], spec[2], epsilon=spec[1], maxRip=maxRip, tabooIteration=taboo,
                          tailcut=tailcut, nthreads=nthreads, **kw)

    loop = run()
    it = loop.res.iter
    before = loop.init if it <= 1 else run(sweep_limit=it - 1).colors
    first = viol_flags(off, idx, before.astype(np.int64))
    order = sorted_color_idx(loop.colors, spec[0]) if tailcut and loop.traj[-1] > 0 else np.arange(spec[0])
    hist = []
    colors, passes, viol = tail_cut_ref(off, idx, loop.colors, first, order, cap, hist, skip_fixed)
    res = CappedResult(it, int(loop.res.maxIterReached), viol, loop.res.glibcDraws, loop.res.initDraws, passes)
    return CappedRun(colors, loop.traj, res, hist, first)


def gap_graph():
    """"gap", n = 2531: G(1000, 0.01) on vertices 0..999, 1100 isolated vertices, G(431, 0.03) on 2100..2530 --
    three list tiles of 1024 vertices, the middle one without an edge, the last of 483 (no multiple of 64)."""
    O.srand(1)
    offa, idxa = O.setup_rnd2(1000, 0.01)
    offb, idxb = O.setup_rnd2(431, 0.03)
    off = np.concatenate([offa, np.full(1100, offa[-1], dtype=np.uint64), offa[-1] + offb[1:]])
    return off.astype(np.uint64), np.concatenate([idxa, idxb + np.uint32(2100)]).astype(np.uint32)
