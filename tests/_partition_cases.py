"""The row-partitioned operator products: partitions, operators, and a restatement of the layout code (a plain module:
no fixtures, no tests).

A row-partitioned product is code of its own: ``remap_cols_kernel`` maps global columns into the chunk-major gathered
operand (``GatherLayout``, common.h), the exchange fills that buffer chunk by chunk, ``tcoow_window_sets`` /
``hipeig_tcoow_plan`` (spmv.hip) sweep a rank's own windows under the exchange and then, per chunk, the windows that chunk
completes.  What a row holds in the end does not depend on the partition: ``slab_cases`` gives one ``pc.RealCase`` per
rank - the slab's rows with global columns, the full operand, ``row_offset`` - so reference and bounds are those of
``_product_cases.py``.

The second half restates the layout code line by line, to be read against the C++: ``pick_gather_chunks`` and
``hipeig_gather_layout`` (comm.hip), ``GatherLayout`` (common.h), the owner search of ``remap_cols_kernel`` and
``tcoow_window_sets`` with the plan decision of ``hipeig_tcoow_plan`` (spmv.hip).  The tests use it to say which plan a
case takes and that the inputs reach what they are meant to reach; tests/test_partitioned_product_cpu.py holds its
properties and a float64 emulation of a rank's product through it.
"""
import functools

import numpy as np

import _product_cases as pc
from eigensolvers_amd.distributed import LoopbackGroup, row_range

MAX_CHUNKS = 4                       # HIPEIG_GATHER_MAX_CHUNKS
SLOT = 16                            # HIPEIG_SLOT_DOUBLES
MAX_RUNS = 4                         # WindowSets::lo / hi: runs per set

# the geometry every partitioned product test forces: N = 9001 has 9 or more column windows, 47 row blocks per 3001 rows
SWEEP_KNOBS = {"HIPEIG_TCOOW_RW": "64", "HIPEIG_TCOOW_WBITS": "10", "HIPEIG_TCOO_RW": "64", "HIPEIG_TCOO_WBITS": "10"}
BLOCK_KNOBS = {"HIPEIG_BCOO_WBITS": "9", "HIPEIG_BCOO_RW": "37"}
WBITS = 10
ALL_KNOBS = tuple(SWEEP_KNOBS) + tuple(BLOCK_KNOBS) + ("HIPEIG_TCOOW_CSPLIT", "HIPEIG_TCOO_PREFETCH", "HIPEIG_GATHER_CHUNKS",
                                                       "HIPEIG_OVERLAP")


# ================================================================ running on ranks
def on_ranks(P, body):
    """``body(rank, ctx)`` on P loopback ranks; the group is closed before anything is looked at.  Every rank's body makes
    the same library calls in the same order (operator creation is collective) and asserts nothing."""
    grp = LoopbackGroup(P)
    try:
        return grp.run(body)
    finally:
        grp.close()


# ================================================================ partitions and operators
N = 9001
PARTITIONS = {
    "balanced2": (N, tuple(row_range(N, 2, r)[0] for r in range(2)) + (N,)),
    "balanced3": (N, tuple(row_range(N, 3, r)[0] for r in range(3)) + (N,)),
    "unequal3": (N, (0, 17, 6000, N)),                       # a 17-row slab, wholly in chunk 0 and shorter than a wave
    "unequal5": (N, (0, 1, 2049, 2050, 7000, N)),            # one-row slabs next to long ones
    "tiny3": (65, tuple(row_range(65, 3, r)[0] for r in range(3)) + (65,)),     # asks for 3 chunks, gets 1
}


def counts_of(cuts):
    return [int(b - a) for a, b in zip(cuts[:-1], cuts[1:])]


@functools.lru_cache(maxsize=None)
def operator(kind, n):
    """``(rowptr, col, val)`` of the n x n operator: ``edge`` - ``pc.edge_matrix`` (two whole row blocks and every 7th row
    empty); ``ragged`` - ``pc.ragged_csr(duplicates=True)``, the arrays as they are (empty and 300-entry rows, unsorted
    columns, a column stored twice)."""
    if kind == "edge":
        A = pc.edge_matrix(n, seed=n)
        return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.copy()
    assert kind == "ragged"
    return pc.ragged_csr(n, 11, duplicates=True) if n >= 600 else _small_ragged(n)


def _small_ragged(n):
    """``ragged_csr`` needs n >= 300 for its long rows; below, rows of 0..12 entries with the same duplicate columns."""
    rng = np.random.default_rng([n, 11])
    lens = rng.integers(0, 13, n)
    lens[rng.choice(n, n // 10, replace=False)] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(n, L, replace=False) for L in lens]).astype(np.int32)
    val = rng.standard_normal(rowptr[-1]) * np.exp(rng.uniform(-3, 3, rowptr[-1]))
    rows = np.arange(0, n, 5)
    rows = rows[lens[rows] >= 2]
    col[rowptr[rows] + 1] = col[rowptr[rows]]
    return rowptr, col, val


def slab_cases(A_csr, x, cuts, name="slab"):
    """One ``pc.RealCase`` per rank: rows ``cuts[r] .. cuts[r + 1]`` with global columns, ``ncols`` = N, ``row_offset`` =
    ``cuts[r]`` and the full operand."""
    rowptr, col, val = A_csr
    n = len(rowptr) - 1
    assert cuts[0] == 0 and cuts[-1] == n and len(x) == n
    out = []
    for r, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        a, b = int(rowptr[lo]), int(rowptr[hi])
        out.append(pc.RealCase(f"{name} rank {r} rows {lo}..{hi}", (rowptr[lo:hi + 1] - rowptr[lo], col[a:b].copy(), val[a:b].copy()),
                               n, lo, x))
    return out


@functools.lru_cache(maxsize=None)
def cases(kind, partition):
    """The slab cases of ``operator(kind)`` on a partition of the table, with ``pc.real_operand`` as the operand."""
    n, cuts = PARTITIONS[partition]
    return tuple(slab_cases(operator(kind, n), pc.real_operand(n, seed=5), cuts, f"{kind} {partition}"))


# ================================================================ the layout code, restated
def pick_gather_chunks(asked, overlap, nranks, max_rows):
    """``pick_gather_chunks`` (comm.hip).  ``asked``: HIPEIG_GATHER_CHUNKS / ``set_gather_chunks`` (0: automatic)."""
    n = asked
    if n <= 0:
        n = 2 if (overlap and nranks > 1 and max_rows >= (8 << 17)) else 1
    if n > MAX_CHUNKS:
        n = MAX_CHUNKS
    while n > 1 and max_rows // n < 16:
        n -= 1
    return n


class GatherLayout:
    """``GatherLayout`` (common.h): [chunk][rank][h], the last chunk's per-rank stride h + 16 (the scalar slots)."""

    def __init__(self, nranks, nchunks, h):
        self.nranks, self.nchunks, self.h = int(nranks), int(nchunks), int(h)
        self.cbase, pos = [], 0
        for k in range(self.nchunks):                       # hipeig_gather_layout's loop
            self.cbase.append(pos)
            pos += self.nranks * self.cstride(k)
        self.cbase += [pos] * (MAX_CHUNKS + 1 - self.nchunks)

    def cstride(self, c):
        return self.h + (SLOT if c == self.nchunks - 1 else 0)

    def pos(self, rank, i):
        c = i // self.h
        if c >= self.nchunks:
            c = self.nchunks - 1
        return self.cbase[c] + rank * self.cstride(c) + (i - c * self.h)

    def slot(self, rank):
        return self.cbase[self.nchunks - 1] + rank * self.cstride(self.nchunks - 1) + self.h

    def total(self):
        return self.cbase[self.nchunks]


def gather_layout(counts, asked=0, overlap=True):
    """``hipeig_gather_layout`` for the ranks' row counts."""
    max_rows = max(counts)
    nch = pick_gather_chunks(asked, overlap, len(counts), max_rows)
    h = (max_rows + nch - 1) // nch
    W = 1 << 17
    if h >= 4 * W:
        h = (h + W - 1) // W * W
    else:
        h = (h + 15) // 16 * 16
    if h < 16:
        h = 16
    return GatherLayout(len(counts), nch, h)


def owner(offs, j):
    """The owner search of ``remap_cols_kernel``: offs[r] <= j < offs[r + 1]."""
    lo, hi = 0, len(offs) - 2
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if j >= offs[mid]:
            lo = mid
        else:
            hi = mid - 1
    return lo


def remap(gl, cuts, col):
    """``remap_cols_kernel`` on an array of global columns (the search vectorised: ``owner`` is what it must equal)."""
    offs = np.asarray(cuts, np.int64)
    col = np.asarray(col, np.int64)
    r = np.searchsorted(offs[1:-1], col, side="right")
    i = col - offs[r]
    c = np.minimum(i // gl.h, gl.nchunks - 1)
    stride = np.where(c == gl.nchunks - 1, gl.h + SLOT, gl.h)
    return np.asarray(gl.cbase, np.int64)[c] + r * stride + (i - c * gl.h)


def operand_positions(gl, counts):
    """Position in the gathered operand of every global row, in row order (``pos`` of every (rank, local row))."""
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return remap(gl, cuts, np.arange(cuts[-1]))


def scatter(gl, counts, x, fill=np.nan):
    """The gathered operand after an exchange: every slice in its places, ``fill`` wherever no operand entry lives."""
    buf = np.full(gl.total(), fill)
    buf[operand_positions(gl, counts)] = x
    return buf


def window_sets(gl, rank, nrows, wbits, nwin):
    """``tcoow_window_sets``: ``sets[0]`` the runs ``(lo, hi)`` of windows wholly inside the rank's own ranges,
    ``sets[1 + k]`` the other windows whose last column belongs to chunk k."""
    W = 1 << wbits
    sets = [[] for _ in range(1 + gl.nchunks)]
    prev_end = 0
    for k in range(gl.nchunks):
        wend = nwin if k == gl.nchunks - 1 else gl.cbase[k + 1] >> wbits
        if wend > nwin:
            wend = nwin
        if wend < prev_end:
            wend = prev_end
        rows_lo = k * gl.h
        rows = min(nrows - rows_lo, gl.h)
        l0 = l1 = 0
        if rows > 0:
            p0 = gl.cbase[k] + rank * gl.cstride(k)
            p1 = p0 + rows
            l0, l1 = (p0 + W - 1) >> wbits, p1 >> wbits
            if l0 < prev_end:
                l0 = prev_end
            if l1 > wend:
                l1 = wend
            if l1 < l0:
                l1 = l0
        if l1 > l0:
            sets[0].append((l0, l1))
            if l0 > prev_end:
                sets[1 + k].append((prev_end, l0))
            if wend > l1:
                sets[1 + k].append((l1, wend))
        elif wend > prev_end:
            sets[1 + k].append((prev_end, wend))
        prev_end = wend
    return sets


def plan(sets, nchunks, overlap=True, fixed=False):
    """The launches of ``hipeig_tcoow_plan`` as lists of window runs, in order; ``None``: the plain exchange and one launch
    over every window (no overlap, the fixed-point form, or nothing to hide the exchange behind)."""
    split = overlap and not fixed
    if split:
        nonempty = sum(1 for s in sets if s)
        if not sets[0] and nchunks == 1:
            split = False
        if nonempty <= 1 and not sets[0]:
            split = False
    return [s for s in sets if s] if split else None


def sets_from_info(info, nranks, rank, nrows):
    """The window sets of a rank from what ``layout_info()`` reports of its blocked copy."""
    gl = GatherLayout(nranks, info["exchange_chunks"], info["rows_per_rank_chunk"])
    return window_sets(gl, rank, nrows, info["window_bits"], info["windows"])


def expected_sets(partition, chunks, overlap=True):
    """Per rank the window sets the restatement gives for a partition of the table at the forced geometry."""
    n, cuts = PARTITIONS[partition]
    counts = counts_of(cuts)
    gl = gather_layout(counts, chunks, overlap)
    nwin = (gl.total() + (1 << WBITS) - 1) >> WBITS
    return gl, [window_sets(gl, r, counts[r], WBITS, nwin) for r in range(len(counts))]
