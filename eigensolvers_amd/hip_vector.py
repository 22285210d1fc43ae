"""``HipVector``: the MI355X backend of the ``AbstractVector`` plugin surface.

It sits beside the reference's ``NumpyVector`` (numpyVector.py:23-238): same constructor
shape ``HipVector(array, options)``, same ``options["linearSystemArgs"]`` keys, same
methods and static hooks, same error behaviour - but the data is a device-resident fp64
buffer and every operation is a call into ``libhipeig.so`` (hand-written gfx950 kernels).
The operator handed to the solver must be a ``HipCsrOperator`` (device-resident CSR);
``HipCsrOperator.from_scipy`` / ``from_dense`` / ``generate`` create one.

With a communicator attached to the context (``HipContext.attach_comm``) a ``HipVector``
holds the LOCAL row slice of a row-partitioned global vector and the same calls become
collective: reductions all-reduce, operator applications all-gather the operand.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib
from .abstract_vector import AbstractVector, LINDEP_DEFAULT_VALUE

_ORTHO_METHODS = {"mgs": 0, "cgs2": 1}
# GCROT solves with a real shift run in lock step (HipVector._solve_real_block) from BLOCK_SOLVE_MIN_GCROT right-hand sides
# on where a vector fits the one-launch Arnoldi batch (n <= gcrotmk._Ops.BATCH_MAX_N), from BLOCK_SOLVE_MIN_GCROT_LONG on
# beyond it (measured: tools/gcrot_block_bench.py, profiles/r06_gcrot_block_bench.jsonl).
BLOCK_SOLVE_MIN_GCROT = 2
BLOCK_SOLVE_MIN_GCROT_LONG = 4
PRECONDITIONER_FLOOR_DEFAULT = 1e-8      # relative; only a guard against h_ii == sigma, not a tuned value


def _preconditioner(o, sigma=None, x0=None, ctx=None, H=None):
    """``o["preconditioner"]`` of a ``linearSystemArgs`` dict, validated: ``None``, ``"jacobi"`` or ``"separable"``.  The
    key belongs to the real-shift single-vector MINRES solve on one GPU; every other combination raises instead of doing
    something else.  ``o["preconditionerLockStep"]`` (``solveBlock``'s lock-step block form of that solve) is validated
    with it: a ``bool``, and ``True`` only together with ``"preconditioner": "jacobi"``.  ``"separable"`` is the
    fast-diagonalisation preconditioner of a ``HipKronSumOperator`` (``H``, where the caller has one at hand);
    ``o["preconditionerPotentials"]`` is validated with it: ``None`` or a list of 1-D arrays, one per mode."""
    pre = o.get("preconditioner")
    lock_step = o.get("preconditionerLockStep", False)
    if not isinstance(lock_step, (bool, np.bool_)):
        raise ValueError(f'linearSystemArgs["preconditionerLockStep"] must be a bool, got {lock_step!r}')
    if lock_step and pre != "jacobi":
        raise ValueError('linearSystemArgs["preconditionerLockStep"] asks for the lock-step block form of the '
                         'preconditioned MINRES: it needs "preconditioner": "jacobi"')
    if pre is None:
        return None
    if pre not in ("jacobi", "separable"):
        raise ValueError(f'linearSystemArgs["preconditioner"] must be None, "jacobi" or "separable", got {pre!r}')
    name = o["linearSolver"]
    if name in ("minres_shifted", "lanczos_filter"):
        raise ValueError(f'linearSystemArgs["preconditioner"] cannot be combined with linearSolver={name!r}: that path takes '
                         "every shift from ONE Krylov space of H, and a preconditioner destroys the shift invariance of "
                         "the Krylov space it rests on")
    if name != "minres":
        raise ValueError(f'linearSystemArgs["preconditioner"] is honoured by linearSolver="minres" only, not {name!r}')
    if sigma is not None and (isinstance(sigma, complex) or np.iscomplexobj(sigma)):
        raise ValueError('linearSystemArgs["preconditioner"] needs a real shift: complex shifts are solved by GCROT, '
                         "which takes no preconditioner here")
    floor = o.get("preconditionerFloor", PRECONDITIONER_FLOOR_DEFAULT)
    if not (isinstance(floor, (int, float, np.floating, np.integer)) and 0.0 <= float(floor) < float("inf")):
        raise ValueError(f'linearSystemArgs["preconditionerFloor"] must be a finite number >= 0, got {floor!r}')
    if x0 is not None:
        raise NotImplementedError("the preconditioned MINRES starts from x = 0: an initial guess (x0) is not implemented "
                                  "with a preconditioner")
    if ctx is not None and ctx.collectives:
        raise NotImplementedError("the preconditioned MINRES runs on one GPU: a context with collectives (a row "
                                  "partition, or its HIPEIG_FORCE_COLLECTIVES rehearsal) is not implemented")
    if pre == "separable":
        pots = o.get("preconditionerPotentials")
        if pots is not None:
            if not isinstance(pots, (list, tuple)) or any(np.ndim(v) != 1 or np.iscomplexobj(v) for v in pots):
                raise ValueError('linearSystemArgs["preconditionerPotentials"] must be None or a list of real 1-D arrays, '
                                 f"one per mode, got {pots!r}")
        if H is not None:
            if not isinstance(H, HipKronSumOperator):
                raise NotImplementedError('linearSystemArgs["preconditioner"] = "separable" diagonalises the factors of a '
                                          f"HipKronSumOperator: {type(H).__name__} has none")
            if pots is not None and [len(v) for v in pots] != list(H.dims):
                raise ValueError(f'linearSystemArgs["preconditionerPotentials"] must hold one array per mode of lengths '
                                 f"{H.dims}, got lengths {[len(v) for v in pots]}")
    return pre


def _gcrot_preconditioner(o, x0=None, ctx=None, H=None):
    """``o["gcrotPreconditioner"]`` of a ``linearSystemArgs`` dict, validated: ``None`` or ``"jacobi"``, the diagonal RIGHT
    preconditioner of the GCROT solves (``HipVector.solve``).  A key of its own: ``"preconditioner"`` belongs to MINRES and
    keeps its refusals.  Returns ``None`` or the relative floor (``o["preconditionerFloor"]``) as a float."""
    pre = o.get("gcrotPreconditioner")
    if pre is None:
        return None
    if pre != "jacobi":
        raise ValueError(f'linearSystemArgs["gcrotPreconditioner"] must be None or "jacobi", got {pre!r}')
    name = o["linearSolver"]
    if name != "gcrotmk":
        raise ValueError(f'linearSystemArgs["gcrotPreconditioner"] is honoured by linearSolver="gcrotmk" only, not {name!r}')
    floor = o.get("preconditionerFloor", PRECONDITIONER_FLOOR_DEFAULT)
    if not (isinstance(floor, (int, float, np.floating, np.integer)) and 0.0 <= float(floor) < float("inf")):
        raise ValueError(f'linearSystemArgs["preconditionerFloor"] must be a finite number >= 0, got {floor!r}')
    if x0 is not None:
        raise NotImplementedError("the preconditioned GCROT starts from x = 0: an initial guess (x0) is not implemented "
                                  "with a preconditioner")
    if ctx is not None and (ctx.collectives or ctx.direct_only):
        raise NotImplementedError("the preconditioned GCROT runs on one GPU: a context with collectives (a row partition, "
                                  "or its HIPEIG_FORCE_COLLECTIVES rehearsal) or a direct-only communicator is not "
                                  "implemented")
    if H is not None and not (isinstance(H, HipCsrOperator) and H.nrows == H.ncols and H.row_offset == 0):
        raise NotImplementedError("the preconditioned GCROT needs a whole HipCsrOperator (nrows == ncols, row_offset == 0): "
                                  "its diagonal is the preconditioner")
    return float(floor)


def _need_block_sweeps(H, what):
    """An explicit opt-in that rests on block sweeps, on an operator that has none: ``NotImplementedError`` naming it."""
    if isinstance(H, HipCsrOperator) and not H.supports_block_sweeps:
        raise NotImplementedError(f"{what} needs block sweeps, which {type(H).__name__} does not have: its products and "
                                  "solves run vector by vector")


def _ptr_table(bufs):
    arr = (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])
    return C.cast(arr, C.POINTER(C.c_void_p)), arr


def _ptr_table_or_null(bufs):
    arr = (C.c_void_p * len(bufs))(*[None if b is None else b.ptr for b in bufs])
    return C.cast(arr, C.POINTER(C.c_void_p)), arr


class HipContext:
    """Owns the device context handle (streams, workspaces, optional RCCL communicator)."""

    _default = None

    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        h = C.c_void_p()
        _lib.call("hipeig_ctx_create", int(device), C.byref(h))
        self.handle = h
        self.device = int(device)
        self.nranks, self.rank = 1, 0
        self.direct_only = False         # a communicator without RCCL (attach_direct_only): no exchange for block operands
        self.partitioned = True          # False in replica mode (set_partitioned): whole operators / vectors on every rank
        self._force_collectives = None   # HIPEIG_FORCE_COLLECTIVES as the library read it when a communicator was attached
        self._pool = {}
        self._finalizer = weakref.finalize(self, HipContext._destroy, h, self._pool)

    @staticmethod
    def _destroy(handle, pool):
        lib = _lib.load()
        for ptrs in pool.values():
            for p in ptrs:
                lib.hipeig_vec_free(handle, C.c_void_p(p))
        pool.clear()
        lib.hipeig_ctx_destroy(handle)

    @classmethod
    def default(cls):
        if cls._default is None:
            cls._default = cls()
        return cls._default

    # ---- communicator -------------------------------------------------------------
    @staticmethod
    def new_unique_id():
        buf = C.create_string_buffer(128)
        _lib.call("hipeig_comm_unique_id", C.cast(buf, C.c_void_p))
        return bytes(buf.raw)

    def attach_comm(self, nranks, rank, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _lib.call("hipeig_comm_init", self.handle, int(nranks), int(rank), C.cast(buf, C.c_void_p))
        self.nranks, self.rank = int(nranks), int(rank)
        self._note_comm()

    def attach_loopback(self, group_handle, nranks, rank):
        """Join an in-process loopback group (``distributed.LoopbackGroup``)."""
        _lib.call("hipeig_comm_init_loopback", self.handle, group_handle, int(rank))
        self.nranks, self.rank = int(nranks), int(rank)
        self._note_comm()

    def _note_comm(self):
        self._force_collectives = os.environ.get("HIPEIG_FORCE_COLLECTIVES", "0") not in ("", "0")

    @property
    def collectives(self):
        """Products and reductions go through the communicator: a row-partitioned run of several ranks, or one rank with
        HIPEIG_FORCE_COLLECTIVES=1 at attach time (the library's flag, comm.hip)."""
        return (self._force_collectives is not None and self.partitioned
                and (self.nranks > 1 or self._force_collectives))

    # ---- operand exchange of a row-partitioned product -------------------------------------------
    GATHER_BACKENDS = {0: "rccl", 1: "direct"}

    def direct_alloc(self, capacity_doubles):
        """This rank's buffers for the direct exchange; returns its 192-byte record (two hipIpc handles + PCI bus id)."""
        buf = C.create_string_buffer(192)
        _lib.call("hipeig_direct_alloc", self.handle, int(capacity_doubles), C.cast(buf, C.c_void_p))
        return bytes(buf.raw)

    def direct_attach(self, records):
        """Map the peers' buffers: ``records`` = every rank's 192-byte record in rank order."""
        blob = b"".join(records)
        buf = C.create_string_buffer(blob, len(blob))
        _lib.call("hipeig_direct_attach", self.handle, C.cast(buf, C.c_void_p))

    def direct_release(self):
        """Free the buffers of the direct exchange (after a collective fall-back to RCCL)."""
        _lib.call("hipeig_direct_release", self.handle)

    def set_direct_wait_limit(self, seconds):
        """Wall-clock limit of the direct exchange's bounded waits from now on (<= 0: the default)."""
        _lib.call("hipeig_comm_set_wait_limit", self.handle, float(seconds))

    def set_exchange(self, on):
        """Measurement aid: ``False`` makes this context's products skip the operand exchange (own slice only; results
        meaningless) so that one rank's sweeps can be timed alone; switch back before the next collective product."""
        _lib.call("hipeig_comm_set_exchange", self.handle, 1 if on else 0)

    def attach_direct_only(self, nranks, rank):
        """A communicator without RCCL (rank / size only): every exchange goes through the direct peer-write backend,
        which must be attached before the first operator is created (``distributed.attach_direct``)."""
        _lib.call("hipeig_comm_init_direct", self.handle, int(nranks), int(rank))
        self.nranks, self.rank = int(nranks), int(rank)
        self.direct_only = True
        self._note_comm()

    def set_gather_backend(self, name):
        code = {v: k for k, v in self.GATHER_BACKENDS.items()}[name]
        _lib.call("hipeig_comm_set_gather_backend", self.handle, code)

    def set_allreduce_backend(self, name):
        code = {v: k for k, v in self.GATHER_BACKENDS.items()}[name]
        _lib.call("hipeig_comm_set_allreduce_backend", self.handle, code)

    def set_gather_chunks(self, nchunks):
        """Chunks of the operand exchange (1-4; 0 = automatic) for operators created from now on (same on every rank)."""
        _lib.call("hipeig_comm_set_gather_chunks", self.handle, int(nchunks))

    def gather_info(self):
        info = (C.c_int64 * 8)()
        _lib.call("hipeig_comm_gather_info", self.handle, info)
        return {"backend": self.GATHER_BACKENDS[int(info[0])], "direct_attached": bool(info[1]), "capacity": int(info[2]),
                "exchanges": int(info[3]), "wait_error": int(info[4]), "chunks_override": int(info[5]),
                "allreduce_backend": self.GATHER_BACKENDS[int(info[6])]}

    def phase_timing(self, on):
        _lib.call("hipeig_phase_timing", self.handle, 1 if on else 0)

    def phase_times(self):
        """ms of the most recent partitioned product: exchange, own-window sweep, remaining sweep, whole product, idle gap
        (None where the phase did not occur)."""
        out = (C.c_double * 8)()
        _lib.call("hipeig_phase_get", self.handle, out)
        names = ("gather_ms", "local_sweep_ms", "remote_sweep_ms", "product_ms", "idle_before_first_chunk_ms")
        return {k: (float(out[i]) if out[i] >= 0 else None) for i, k in enumerate(names)}

    def allreduce_ms(self, count=2, reps=50):
        out = C.c_double()
        _lib.call("hipeig_comm_bench_allreduce", self.handle, int(count), int(reps), C.byref(out))
        return float(out.value)

    def set_partitioned(self, flag):
        """False: replica mode - whole operators and vectors on every rank, no implicit collectives;
        only ``allreduce_vector`` exchanges data (FEAST contour replicas)."""
        _lib.call("hipeig_comm_set_partitioned", self.handle, 1 if flag else 0)
        self.partitioned = bool(flag)

    def allreduce_vector(self, buf):
        """SUM of a device buffer over the ranks, in place."""
        _lib.call("hipeig_vec_allreduce", self.handle, buf.ptr, buf.n)

    # ---- memory -------------------------------------------------------------------
    def alloc(self, n):
        free = self._pool.get(n)
        if free:
            return DeviceBuffer(self, free.pop(), n)
        p = C.c_void_p()
        _lib.call("hipeig_vec_alloc", self.handle, int(n), C.byref(p))
        return DeviceBuffer(self, p.value, n)

    def synchronize(self):
        _lib.call("hipeig_ctx_sync", self.handle)

    def device_info(self):
        info = (C.c_int64 * 8)()
        name = C.create_string_buffer(256)
        _lib.call("hipeig_device_info", self.handle, info, name, 256)
        return {"name": name.value.decode(), "cus": info[0], "wave": info[1], "hbm_total": info[2],
                "hbm_free": info[3], "l2_bytes": info[4]}

    def timer_start(self):
        _lib.call("hipeig_timer_start", self.handle)

    def timer_stop(self):
        ms = C.c_float()
        _lib.call("hipeig_timer_stop", self.handle, C.byref(ms))
        return float(ms.value)


class DeviceBuffer:
    """A device allocation of n doubles; returned to the context's pool when collected.

    All work is ordered on one stream, so recycling a buffer without a sync is safe."""

    __slots__ = ("ctx", "ptr", "n", "__weakref__")

    def __init__(self, ctx, ptr, n):
        self.ctx, self.ptr, self.n = ctx, ptr, n

    def __del__(self):
        try:
            self.ctx._pool.setdefault(self.n, []).append(self.ptr)
        except Exception:
            pass


class HipCsrOperator:
    """Device-resident sparse symmetric operator (local rows of a row partition)."""

    # Block sweeps (block products, lock-step solves, the Lanczos filter) exist for this operator: consulted wherever a
    # lock-step path is chosen, so that an operator without them takes the one-by-one calls.
    supports_block_sweeps = True

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.handle = handle
        info = (C.c_int64 * 8)()
        _lib.call("hipeig_csr_info", handle, info)
        self.nrows, self.ncols, self.nnz, self.row_offset = info[0], info[1], info[2], info[3]
        self.device_bytes = info[5]
        self.shape = (self.nrows, self.ncols)
        self.dtype = np.dtype(np.float64)
        self._finalizer = weakref.finalize(self, HipCsrOperator._destroy, ctx, handle)

    @staticmethod
    def _destroy(ctx, handle):
        _lib.load().hipeig_csr_destroy(ctx.handle, handle)

    @classmethod
    def from_csr_arrays(cls, rowptr, col, val, ncols, row_offset=0, ctx=None):
        if np.iscomplexobj(val):
            raise TypeError("HipCsrOperator holds real fp64 operators")
        ctx = ctx or HipContext.default()
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        h = C.c_void_p()
        _lib.call("hipeig_csr_create", ctx.handle, len(rowptr) - 1, int(ncols), int(row_offset),
                  rowptr.ctypes.data_as(C.POINTER(C.c_int64)), col.ctypes.data_as(C.POINTER(C.c_int32)),
                  val.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
        return cls(ctx, h)

    @classmethod
    def from_scipy(cls, A, row_begin=0, row_end=None, ctx=None):
        """Upload rows [row_begin,row_end) of a scipy.sparse matrix (real, any format)."""
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        if np.iscomplexobj(A.data):
            raise TypeError("HipCsrOperator holds real fp64 operators")
        row_end = A.shape[0] if row_end is None else row_end
        sl = A[row_begin:row_end]
        return cls.from_csr_arrays(sl.indptr, sl.indices, sl.data, A.shape[1], row_begin, ctx)

    @classmethod
    def from_dense(cls, M, ctx=None, layout=None):
        """Dense ndarray stored as a full CSR (every entry kept) - plumbing-size problems.  ``layout="dense"`` also pins
        the operator to the dense row sweeps (``set_variant(6)``, ``set_block_variant(3)``): a row-major fp64 copy, built
        on the device at the first product, 8 bytes per entry and no gathers.  ``layout=None`` keeps the automatic choice."""
        if layout not in (None, "dense"):
            raise ValueError(f'layout must be None or "dense", got {layout!r}')
        if np.iscomplexobj(M):
            raise TypeError("HipCsrOperator holds real fp64 operators")
        M = np.asarray(M, dtype=np.float64)
        n, m = M.shape
        rowptr = np.arange(0, n * m + 1, m, dtype=np.int64)
        col = np.tile(np.arange(m, dtype=np.int32), n)
        H = cls.from_csr_arrays(rowptr, col, M.ravel(), m, 0, ctx)
        if layout == "dense":
            H.set_variant(6)
            H.set_block_variant(3)
        return H

    @classmethod
    def generate(cls, N, nnz_row=64, seed=7, row_begin=0, row_end=None, ctx=None, **kw):
        """Synthetic gapped random-sparse Hermitian operator built on the device
        (bit-identical to ``generators.gapped_csr_host``)."""
        from .generators import gapped_params
        ctx = ctx or HipContext.default()
        p = gapped_params(N, nnz_row, seed, **kw)
        row_end = N if row_end is None else row_end
        t = np.ascontiguousarray(p["targets"], dtype=np.float64)
        h = C.c_void_p()
        _lib.call("hipeig_csr_generate", ctx.handle, int(N), int(row_begin), int(row_end), p["K"],
                  C.c_uint64(p["seed"]), p["eps"], C.c_uint32(p["thresh24"]),
                  t.ctypes.data_as(C.POINTER(C.c_double)), len(t), C.byref(h))
        return cls(ctx, h)

    def diagonal(self):
        """Device buffer with ``d_i`` = the sum of the stored ``(i, i)`` entries of local row ``i`` (0 where a row stores
        none; duplicate entries are separate stored elements and are summed in stored order).  Taken once per operator."""
        d = getattr(self, "_diagonal", None)
        if d is None:
            d = self.ctx.alloc(self.nrows)
            _lib.call("hipeig_csr_diagonal", self.ctx.handle, self.handle, d.ptr)
            self._diagonal = d
        return d

    def jacobi_inverse(self, sigma, floor=PRECONDITIONER_FLOOR_DEFAULT):
        """Device buffer with ``minv_i = 1 / max(t_i, floor * max_j t_j)``, ``t_i = |sigma - d_i|``: the ``M^-1`` of the
        Jacobi-preconditioned MINRES.  Kept for the latest ``(sigma, floor)``: a Lanczos run has one shift, so it is built
        once.  ``ValueError`` where an element would not be finite (``h_ii == sigma`` with ``floor = 0``)."""
        key = (float(sigma), float(floor))
        cached = getattr(self, "_jacobi", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        d = self.diagonal()
        minv = self.ctx.alloc(self.nrows)
        try:
            _lib.call("hipeig_jacobi_inverse", self.ctx.handle, self.nrows, d.ptr, key[0], key[1], minv.ptr)
        except _lib.HipEigError as exc:
            if "not finite" in str(exc):
                raise ValueError(str(exc)) from None
            raise
        self._jacobi = (key, minv)
        return minv

    JACOBI_Z_CACHE = 16      # entries (16 n bytes each) of jacobi_inverse_z's cache: the contour points of a FEAST run recur
                             # every iteration, and a pool holds at most gcrotmk.POOL_MAX_WIDTH = 16 of them at once

    def jacobi_inverse_z(self, z, floor=PRECONDITIONER_FLOOR_DEFAULT):
        """``(minv_re, minv_im)`` device buffers of GCROT's diagonal right preconditioner ``M^-1 = diag(1 / (z - d_i))`` for
        a real shift or a complex contour point ``z``, kept away from ``d_i == z`` by the relative ``floor``
        (``hipeig_jacobi_inverse_z``; ``precond_gcrotmk.jacobi_inverse_z_host`` is its NumPy statement).  ``minv_im`` is
        ``None`` for a real ``z``.  Unlike ``jacobi_inverse`` it keeps sign and phase.  The latest ``JACOBI_Z_CACHE``
        ``(complex(z), floor)`` are kept, least recently used dropped first.  ``ValueError`` where an element would not be
        finite (``d_i == z`` with ``floor = 0``), ``d`` is not finite or every ``|z - d_i|`` is 0."""
        if not (self.nrows == self.ncols and self.row_offset == 0):
            raise NotImplementedError("jacobi_inverse_z needs a whole operator (nrows == ncols, row_offset == 0)")
        z = complex(z)
        key = (z, float(floor))
        cache = self.__dict__.setdefault("_jacobi_z", {})
        if key in cache:
            cache[key] = cache.pop(key)                  # most recently used last
            return cache[key]
        d = self.diagonal()
        re = self.ctx.alloc(self.nrows)
        im = self.ctx.alloc(self.nrows) if z.imag != 0.0 else None
        try:
            _lib.call("hipeig_jacobi_inverse_z", self.ctx.handle, self.nrows, d.ptr, z.real, z.imag, key[1], re.ptr,
                      None if im is None else im.ptr)
        except _lib.HipEigError as exc:
            if "not finite" in str(exc):
                raise ValueError(str(exc)) from None
            raise
        while len(cache) >= self.JACOBI_Z_CACHE:
            del cache[next(iter(cache))]
        cache[key] = (re, im)
        return cache[key]

    VARIANTS = {0: "none", 1: "csr-vector", 2: "csr-stream", 3: "column-window-blocked(wave)",
                4: "column-window-blocked(workgroup)", 5: "column-window-blocked(workgroup, fixed-point)", 6: "dense"}

    def set_variant(self, variant):
        """Operator kernel: 0 automatic; 1 CSR-vector, 2 CSR-stream, 3 column-window blocked with wave-owned rows
        (these three fix the order of the adds inside a row: bitwise reproducible); 4 column-window blocked with
        workgroup-owned rows and fp64 LDS atomics (the fast default for large operators; a row's sum is
        reproducible to rounding only); 5 the same sweep with FIXED-POINT accumulators - integer adds commute, so
        it is bitwise reproducible at the speed of 4, with an absolute error per row of
        ~nnz_row * 2^-61 * max_i sum_j|a_ij| * max|x| instead of fp64's relative one; 6 the dense row sweep on a
        row-major fp64 copy built at the first product (``dense_info``): no column indices, no gathers, a row's adds in
        an order that depends on the number of columns only (bitwise reproducible).  Opt-in: the automatic choice never
        takes it.  It needs a whole square operator on a context without a communicator and a copy that fits the free
        device memory; anything else is refused with a message, here or at the first product, never replaced."""
        _lib.call("hipeig_csr_set_variant", self.handle, int(variant))
        self._variant = int(variant)

    def honour_reduction_option(self, options):
        """``options["reduction"]`` of the vectors: "deterministic" restricts the operator to
        bitwise reproducible kernels - on the automatic choice CSR-stream stays, the fixed-point variant 5 takes the
        place of the fp64-atomic variant 4 (same speed) and block products take the row-owner kernel; an operator
        pinned to 4 moves to 5.  "fast" undoes both.  An explicitly pinned variant 1-3 or 6 (fixed-order kernels) is left
        alone."""
        want = (options or {}).get("reduction")
        if want not in (None, "deterministic", "fast"):
            raise ValueError(f'options["reduction"] must be "deterministic" or "fast", got {want!r}')
        if want is None or want == getattr(self, "_reduction", None):
            return
        if getattr(self, "_reduction_pinned", False):
            return                                   # set_reduction() on the operator wins over per-vector options
        if getattr(self, "_reduction", None) is not None:
            # the mode is a property of the OPERATOR (its kernels), shared by every vector that uses it: two vectors asking
            # for different modes would flip the kernels back and forth under each other
            raise ValueError(f'this operator already runs with reduction={self._reduction!r} (asked for by another vector); '
                             f'a vector with reduction={want!r} needs its own operator, or settle it with H.set_reduction()')
        cur = getattr(self, "_variant", 0)
        _lib.call("hipeig_csr_set_reproducible", self.handle, 1 if want == "deterministic" else 0)
        if want == "deterministic" and cur == 4:
            self.set_variant(5)
            self._moved_by_option = True
        elif want == "fast" and cur == 5 and getattr(self, "_moved_by_option", False):
            self.set_variant(4)
            self._moved_by_option = False
        self._reduction = want

    def set_reduction(self, mode):
        """Pin the reduction mode of this operator ("deterministic": bitwise reproducible kernels only; "fast"; None: back to
        what the vectors' options ask for) whatever ``options["reduction"]`` later vectors carry."""
        self._reduction_pinned = False
        previous, self._reduction = getattr(self, "_reduction", None), None
        if mode is None:
            if previous == "deterministic":              # back to the unrestricted kernels, then forget
                self.honour_reduction_option({"reduction": "fast"})
                self._reduction = None
            return
        self.honour_reduction_option({"reduction": mode})
        self._reduction_pinned = True

    def fixed_point_info(self):
        """(max_i sum_j |a_ij|, max |x| of the last variant-5 operand): what bounds variant 5's absolute error."""
        out = (C.c_double * 2)()
        _lib.call("hipeig_csr_fixed_info", self.ctx.handle, self.handle, out)
        return float(out[0]), float(out[1])

    def last_variant(self):
        """Name of the kernel variant the most recent product used."""
        info = (C.c_int64 * 8)()
        _lib.call("hipeig_csr_info", self.handle, info)
        return self.VARIANTS[int(info[4])]

    BLOCK_VARIANTS = {0: "none", 1: "row-owner", 2: "column-window-blocked", 3: "dense"}

    def set_block_variant(self, variant):
        """Kernel of the block product / block solve: 0 automatic, 1 row-owner CSR, 2 window-blocked, 3 the dense block
        sweep on the copy of variant 6 (opt-in, refused under the same conditions)."""
        _lib.call("hipeig_csr_set_block_variant", self.handle, int(variant))

    def block_info(self):
        info = (C.c_int64 * 4)()
        _lib.call("hipeig_csr_block_info", self.handle, info)
        return {"variant": self.BLOCK_VARIANTS[int(info[0])], "row_blocks": int(info[1]), "windows": int(info[2]),
                "rows_per_block": int(info[3])}

    def dense_info(self):
        """The dense copy of variant 6 / block variant 3: rows, columns, ``ld`` (doubles per row: the columns rounded up to
        a 128-byte line), ``bytes`` of the copy (0 until the first dense product built it), rows a wave carries per pass and
        the workgroups of the last dense single-vector / block launch.  Refreshes ``device_bytes``."""
        out = (C.c_int64 * 8)()
        _lib.call("hipeig_csr_dense_info", self.handle, out)
        info = (C.c_int64 * 8)()
        _lib.call("hipeig_csr_info", self.handle, info)
        self.device_bytes = info[5]
        keys = ("rows", "cols", "ld", "bytes", "rows_per_wave", "workgroups", "block_workgroups")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def dense_algorithmic_bytes(self):
        """Bytes one dense product has to move: the matrix once, x once, y once."""
        return 8 * self.nrows * self.ncols + 8 * self.ncols + 8 * self.nrows

    def layout_info(self):
        """Layout constants of the blocked copy the last product ran on (a counter profile is valid for these only)."""
        out = (C.c_int64 * 13)()
        _lib.call("hipeig_csr_layout_info", self.handle, out)
        keys = ("variant", "rows_per_block", "window_bits", "row_blocks", "windows", "column_splits", "workgroups_per_launch",
                "threads", "unroll", "exchange_chunks", "rows_per_rank_chunk", "bins")
        info = {k: int(out[i]) for i, k in enumerate(keys)}
        if out[12] > 0:                    # workgroup-unit stream: slots (padding included) per non-zero
            info["padding"] = round(int(out[12]) / max(1, self.nnz), 5)
        return info

    def launches_per_apply(self):
        """Kernel launches (sweeps) one product takes with the variant last used."""
        info = (C.c_int64 * 8)()
        _lib.call("hipeig_csr_info", self.handle, info)
        return max(1, int(info[7]))

    def to_scipy(self):
        import scipy.sparse as sp
        rp = np.empty(self.nrows + 1, dtype=np.int64)
        col = np.empty(self.nnz, dtype=np.int32)
        val = np.empty(self.nnz, dtype=np.float64)
        _lib.call("hipeig_csr_download", self.ctx.handle, self.handle,
                  rp.ctypes.data_as(C.POINTER(C.c_int64)), col.ctypes.data_as(C.POINTER(C.c_int32)),
                  val.ctypes.data_as(C.POINTER(C.c_double)))
        return sp.csr_matrix((val, col, rp), shape=(self.nrows, self.ncols))

    def algorithmic_bytes(self):
        """nnz*(8+4) + (nrows+1)*4 + 8*ncols (x once) + 8*nrows (y)."""
        return self.nnz * 12 + (self.nrows + 1) * 4 + 8 * self.ncols + 8 * self.nrows

    # y = H x on raw buffers
    def apply(self, x, y):
        _lib.call("hipeig_spmv", self.ctx.handle, self.handle, x.ptr, y.ptr)

    def apply_block(self, xs):
        """[H x for x in xs] as one block product (tall-skinny SpMM); xs are DeviceBuffers."""
        ys = [self.ctx.alloc(self.nrows) for _ in xs]
        xt, keep1 = _ptr_table(xs)
        yt, keep2 = _ptr_table(ys)
        _lib.call("hipeig_spmm", self.ctx.handle, self.handle, len(xs), xt, yt)
        return ys

    def apply_shifted(self, sigma, x, y, reverse=False):
        _lib.call("hipeig_spmv_shift", self.ctx.handle, self.handle, float(sigma),
                  -1.0 if reverse else 1.0, x.ptr, y.ptr)

    def apply_shifted_block(self, sigma, xs, reverse=False):
        """[sign*(sigma*x - H x) for x in xs] for real operands and a real shift (the operator of the lock-step GCROT
        solves): eight operands share one pass over the operator (``hipeig_spmm_shift``).  Returns new buffers."""
        ys = [self.ctx.alloc(self.nrows) for _ in xs]
        xt, keep1 = _ptr_table(xs)
        yt, keep2 = _ptr_table(ys)
        _lib.call("hipeig_spmm_shift", self.ctx.handle, self.handle, len(xs), float(sigma), -1.0 if reverse else 1.0, xt, yt)
        return ys

    def apply_shifted_pair(self, z, xr, xi, yr, yi, reverse=False):
        """(yr, yi) = sign*(z*x - H x) for the complex operand x = xr + i xi and the complex shift z (the operator is
        real): one sweep of the operator for both halves on large operators (``hipeig_spmv_shift_pair``)."""
        z = complex(z)
        _lib.call("hipeig_spmv_shift_pair", self.ctx.handle, self.handle, z.real, z.imag,
                  -1.0 if reverse else 1.0, xr.ptr, xi.ptr, yr.ptr, yi.ptr)

    def apply_shifted_pairs(self, z, xs, reverse=False):
        """[sign*(z*x - H x) for x in xs] for complex operands xs = [(re, im) DeviceBuffers, ...]: four operands share one
        pass over the operator (``hipeig_spmm_shift_pairs``).  ``z``: one shift, or a sequence of ``len(xs)`` shifts, one per
        operand (``hipeig_spmm_shift_pairs_z``: operands of different contour points in one block).  Returns new (re, im)
        buffer pairs."""
        per_operand = np.ndim(z) > 0
        if per_operand:
            zs = np.asarray(z, dtype=np.complex128).reshape(-1)
            if len(zs) != len(xs):
                raise ValueError(f"{len(zs)} shifts for {len(xs)} operands")
        else:
            z = complex(z)
        n = self.nrows
        ys = [(self.ctx.alloc(n), self.ctx.alloc(n)) for _ in xs]
        t_xr, k1 = _ptr_table([x[0] for x in xs])
        t_xi, k2 = _ptr_table([x[1] for x in xs])
        t_yr, k3 = _ptr_table([y[0] for y in ys])
        t_yi, k4 = _ptr_table([y[1] for y in ys])
        if per_operand:
            zr, zi = np.ascontiguousarray(zs.real), np.ascontiguousarray(zs.imag)
            DP = C.POINTER(C.c_double)
            _lib.call("hipeig_spmm_shift_pairs_z", self.ctx.handle, self.handle, len(xs), zr.ctypes.data_as(DP),
                      zi.ctypes.data_as(DP), -1.0 if reverse else 1.0, t_xr, t_xi, t_yr, t_yi)
            return ys
        _lib.call("hipeig_spmm_shift_pairs", self.ctx.handle, self.handle, len(xs), z.real, z.imag, -1.0 if reverse else 1.0,
                  t_xr, t_xi, t_yr, t_yi)
        return ys

    # ---- products of the diagonally right-preconditioned GCROT solves: the same with minv (.) x in place of x --------------
    def diag_mul(self, minv, x, y=None):
        """``y = minv (.) x`` for a real ``x`` (a DeviceBuffer) or a complex one (a ``(re, im)`` pair) and a ``minv`` as
        ``jacobi_inverse_z`` returns it; a real ``x`` needs a real ``minv``.  ``y``: where to (may be ``x``), default new
        buffers.  Returns ``y``."""
        n = self.nrows
        if isinstance(x, tuple):
            y = (self.ctx.alloc(n), self.ctx.alloc(n)) if y is None else y
            _lib.call("hipeig_pair_diag_mul", self.ctx.handle, n, minv[0].ptr, None if minv[1] is None else minv[1].ptr,
                      x[0].ptr, x[1].ptr, y[0].ptr, y[1].ptr)
            return y
        if minv[1] is not None:
            raise ValueError("a real operand takes a real minv")
        y = self.ctx.alloc(n) if y is None else y
        _lib.call("hipeig_diag_mul", self.ctx.handle, n, minv[0].ptr, x.ptr, y.ptr)
        return y

    def apply_shifted_m(self, sigma, minv, x, y, reverse=False):
        """``y = sign*(sigma*t - H t)``, ``t = minv (.) x``: one scaling, then ``apply_shifted``."""
        self.apply_shifted(sigma, self.diag_mul(minv, x), y, reverse=reverse)

    def apply_shifted_block_m(self, sigma, minv, xs, reverse=False):
        """``apply_shifted_block`` on ``minv (.) x``, scaled while the operands are packed (``hipeig_spmm_shift_m``)."""
        ys = [self.ctx.alloc(self.nrows) for _ in xs]
        xt, keep1 = _ptr_table(xs)
        yt, keep2 = _ptr_table(ys)
        _lib.call("hipeig_spmm_shift_m", self.ctx.handle, self.handle, len(xs), float(sigma), -1.0 if reverse else 1.0,
                  minv[0].ptr, xt, yt)
        return ys

    def apply_shifted_pairs_m(self, zs, minvs, xs, reverse=False):
        """``apply_shifted_pairs`` with a shift AND a ``minv`` per operand, ``[sign*(z_p*t_p - H t_p)]`` with
        ``t_p = minv_p (.) x_p`` scaled while the operands are packed (``hipeig_spmm_shift_pairs_zm``); one operand is one
        scaling and the single pair product."""
        zs = np.asarray(zs, dtype=np.complex128).reshape(-1)
        if not (len(zs) == len(xs) == len(minvs)):
            raise ValueError(f"{len(zs)} shifts and {len(minvs)} minv for {len(xs)} operands")
        n = self.nrows
        ys = [(self.ctx.alloc(n), self.ctx.alloc(n)) for _ in xs]
        t_mr, k0 = _ptr_table([m[0] for m in minvs])
        t_mi, k00 = _ptr_table_or_null([m[1] for m in minvs])
        t_xr, k1 = _ptr_table([x[0] for x in xs])
        t_xi, k2 = _ptr_table([x[1] for x in xs])
        t_yr, k3 = _ptr_table([y[0] for y in ys])
        t_yi, k4 = _ptr_table([y[1] for y in ys])
        zr, zi = np.ascontiguousarray(zs.real), np.ascontiguousarray(zs.imag)
        DP = C.POINTER(C.c_double)
        _lib.call("hipeig_spmm_shift_pairs_zm", self.ctx.handle, self.handle, len(xs), zr.ctypes.data_as(DP),
                  zi.ctypes.data_as(DP), -1.0 if reverse else 1.0, t_mr, t_mi, t_xr, t_xi, t_yr, t_yi)
        return ys

    def apply_pair(self, xr, xi, yr, yi):
        """(yr, yi) = (H xr, H xi): ``applyOp`` on a complex vector, one sweep where the pair kernel applies."""
        _lib.call("hipeig_spmv_shift_pair", self.ctx.handle, self.handle, 0.0, 0.0, 0.0, xr.ptr, xi.ptr, yr.ptr, yi.ptr)

    def pair_info(self):
        """{'fused': the most recent pair product ran as one sweep, 'launches': its sweep launches}"""
        out = (C.c_int64 * 2)()
        _lib.call("hipeig_csr_pair_info", self.handle, out)
        return {"fused": bool(out[0]), "launches": int(out[1])}

    def __matmul__(self, v):
        if isinstance(v, HipVector):
            return v.applyOp(self)
        return NotImplemented


class HipKronSumOperator(HipCsrOperator):
    """Kronecker-sum operator on a direct-product grid, applied factor by factor on the matrix cores::

        H = sum_d  I_(n_1..n_{d-1}) (x) T_d (x) I_(n_{d+1}..n_D)  +  diag(V),      N = n_1 * ... * n_D

    with dense ``n_d x n_d`` factors and a general diagonal ``V`` (where the modes couple): the vibrational Hamiltonians in
    a product / DVR basis.  The vector index is in C order, last mode fastest: ``r = ((i_1 n_2 + i_2) n_3 + ...) + i_D``.
    As a ``HipCsrOperator`` it passes every gate of the solvers; what a single vector does with an operator - ``applyOp``,
    ``matrixRepresentation``, ``solve`` with ``minres`` (plain, Jacobi), ``minres_shifted`` and ``gcrotmk``, the Lanczos
    and FEAST drivers - is inherited.  Block sweeps are not built (``supports_block_sweeps``):
    ``solveBlock`` and every automatic lock-step choice solve one by one, ``apply_block`` loops over single products, and
    the explicit opt-ins that need them raise ``NotImplementedError``.  A row's adds are in an order the dims alone fix:
    bitwise reproducible."""

    supports_block_sweeps = False
    VARIANTS = {**HipCsrOperator.VARIANTS, 7: "kronecker-sum"}          # the variant hipeig_kron_create pins; it cannot be set
    MAX_MODES = 8
    KERNEL_FORMS = {1: "mfma", 2: "mfma-last", 3: "plain"}

    def __init__(self, ctx, handle, factors, diag):
        super().__init__(ctx, handle)
        self._finalizer.detach()
        self._finalizer = weakref.finalize(self, HipKronSumOperator._destroy, ctx, handle)
        self._factors = factors
        self._diag = diag
        self.dims = tuple(int(t.shape[0]) for t in factors)
        self._variant = 7

    @staticmethod
    def _destroy(ctx, handle):
        _lib.load().hipeig_kron_destroy(ctx.handle, handle)

    @staticmethod
    def _checked(factors, diag, check):
        """The host side of ``from_factors``: ``(factors, V or None)`` as contiguous fp64 arrays, or the refusal."""
        factors = list(factors)
        if not 1 <= len(factors) <= HipKronSumOperator.MAX_MODES:
            raise ValueError(f"a Kronecker sum takes 1 to {HipKronSumOperator.MAX_MODES} factors, got {len(factors)}")
        out = []
        for d, T in enumerate(factors, 1):
            if np.iscomplexobj(T):
                raise TypeError("HipKronSumOperator holds real fp64 factors")
            T = np.ascontiguousarray(T, dtype=np.float64)
            if T.ndim != 2 or T.shape[0] != T.shape[1] or T.shape[0] < 1:
                raise ValueError(f"factor {d} is not a square matrix: shape {T.shape}")
            if check:
                if not np.all(np.isfinite(T)):
                    raise ValueError(f"factor {d} is not finite")
                if np.max(np.abs(T - T.T)) > 1e-12 * np.max(np.abs(T)):
                    raise ValueError(f"factor {d} is not symmetric to 1e-12 * max|T| (check=False applies it as given)")
            out.append(T)
        dims = tuple(T.shape[0] for T in out)
        N = int(np.prod([int(n) for n in dims], dtype=object))
        if N >= 2 ** 31:
            raise ValueError(f"N = {N} does not stay below 2^31")
        V = None
        if diag is not None:
            if np.iscomplexobj(diag):
                raise TypeError("HipKronSumOperator holds a real fp64 diagonal")
            V = np.asarray(diag, dtype=np.float64)
            if V.shape != dims and V.shape != (N,):
                raise ValueError(f"diag has shape {V.shape}: expected {dims} or ({N},)")
            V = np.ascontiguousarray(V.reshape(N))
            if check and not np.all(np.isfinite(V)):
                raise ValueError("diag is not finite")
        return out, V

    @classmethod
    def from_factors(cls, factors, diag=None, ctx=None, check=True):
        """``factors``: the ``T_d``, dense and square, ``1 <= D <= 8``, ``n_d >= 1``, ``N < 2^31``; ``diag``: ``None``, an
        array of shape ``dims`` or of length ``N``.  ``check=True`` raises ``ValueError`` for a factor that is not square,
        not finite or not symmetric to ``1e-12 * max|T_d|``; ``check=False`` applies the factors as given (``T_d[i, k]``,
        not transposed).  A factor larger than the kernels take (``kron_info()["max_factor"]``) and a context with a
        communicator are refused with a message: there is no slow path."""
        factors, V = cls._checked(factors, diag, check)
        ctx = ctx or HipContext.default()
        if ctx.collectives or ctx.direct_only or ctx.nranks > 1:
            raise ValueError("HipKronSumOperator does not take a context with a communicator (a row partition, its "
                             "HIPEIG_FORCE_COLLECTIVES rehearsal or a direct-only exchange)")
        D = len(factors)
        DP = C.POINTER(C.c_double)
        dims = (C.c_int64 * D)(*[T.shape[0] for T in factors])
        tab = (DP * D)(*[T.ctypes.data_as(DP) for T in factors])
        h = C.c_void_p()
        try:
            _lib.call("hipeig_kron_create", ctx.handle, D, dims, tab, None if V is None else V.ctypes.data_as(DP), C.byref(h))
        except _lib.HipEigError as exc:
            if "status 2" in str(exc):                    # a refusal with a message, not a failure
                raise ValueError(str(exc)) from None
            raise
        return cls(ctx, h, factors, V)

    # ---- what it is ---------------------------------------------------------------------------------------------
    def kron_info(self):
        """Launches per product (one per mode and the one that carries the row epilogue), per mode the kernel form
        (``"mfma"``: matrix cores, inner stride >= 16; ``"mfma-last"``: matrix cores, last mode; ``"plain"``: FMA chain,
        inner stride 2..15 or a singleton mode) and the padded size of the device copy of its factor."""
        out = (C.c_int64 * 40)()
        _lib.call("hipeig_kron_info", self.handle, out)
        D = int(out[0])
        return {"modes": D, "n": int(out[1]), "launches": int(out[2]), "device_bytes": int(out[3]),
                "raw_bytes": int(out[4]), "max_factor": int(out[5]),
                "kernels": [self.KERNEL_FORMS[int(out[8 + 4 * d])] for d in range(D)],
                "padded": [(int(out[10 + 4 * d]), int(out[11 + 4 * d])) for d in range(D)]}

    def algorithmic_bytes(self):
        """Bytes one product has to move: every mode launch reads x, reads the running sums (the first one V, when there
        is one) and writes them, 3 streams of 8 N; the epilogue launch reads the sums and writes y, 2 more; the factors
        once: ``(3 D + 2) * 8 N + 8 sum_d n_d^2``.  An upper bound: on the chip the vector streams of a problem that fits
        the last-level cache do not all reach HBM."""
        N, D = self.nrows, len(self.dims)
        return (3 * D + 2) * 8 * N + 8 * sum(n * n for n in self.dims)

    def diagonal(self):
        """Device buffer with ``sum_d T_d[i_d, i_d] + V``, summed in the order of ``to_scipy()``; built once."""
        d = getattr(self, "_diagonal", None)
        if d is None:
            d = self.ctx.alloc(self.nrows)
            _lib.call("hipeig_kron_diagonal", self.ctx.handle, self.handle, d.ptr)
            self._diagonal = d
        return d

    def _separable_tables(self, potentials=None, bases=None, eigenvalues=None):
        """The device record of one decomposition (``hipeig_kron_precond_create``), kept per potentials: a Lanczos run
        decomposes once.  Given ``bases`` and ``eigenvalues`` are taken as they are and not kept."""
        from .precond_minres import separable_basis_host, separable_fit_host
        if (bases is None) != (eigenvalues is None):
            raise ValueError("bases and eigenvalues are given together")
        D = len(self.dims)
        if bases is None:
            if potentials is None:
                key = None
                potentials = separable_fit_host(self._diag, self.dims)
            else:
                potentials = [np.ascontiguousarray(v, dtype=np.float64) for v in potentials]
                if [v.shape for v in potentials] != [(n,) for n in self.dims]:
                    raise ValueError(f"potentials: one 1-D array per mode of lengths {self.dims}, got shapes "
                                     f"{[v.shape for v in potentials]}")
                key = tuple(v.tobytes() for v in potentials)
            cache = self.__dict__.setdefault("_separable", {})
            if key in cache:
                return cache[key]
            bases, eigenvalues = separable_basis_host(self._factors, potentials)
        else:
            key, cache = None, None
            bases = [np.ascontiguousarray(Q, dtype=np.float64) for Q in bases]
            eigenvalues = [np.ascontiguousarray(lam, dtype=np.float64) for lam in eigenvalues]
            if [Q.shape for Q in bases] != [(n, n) for n in self.dims] or [lam.shape for lam in eigenvalues] != [(n,) for n in self.dims]:
                raise ValueError(f"bases / eigenvalues: one n_d x n_d matrix and one vector of n_d per mode of {self.dims}")
        DP = C.POINTER(C.c_double)
        dims = (C.c_int64 * D)(*self.dims)
        qt = (DP * D)(*[Q.ctypes.data_as(DP) for Q in bases])
        lt = (DP * D)(*[lam.ctypes.data_as(DP) for lam in eigenvalues])
        h = C.c_void_p()
        _lib.call("hipeig_kron_precond_create", self.ctx.handle, self.handle, D, dims, qt, lt, C.byref(h))
        tables = _SeparableTables(self, h, bases, eigenvalues)
        if cache is not None:
            cache[key] = tables
        return tables

    def separable_preconditioner(self, sigma, floor=PRECONDITIONER_FLOOR_DEFAULT, potentials=None, bases=None,
                                 eigenvalues=None):
        """The fast-diagonalisation preconditioner ``M^-1 = Q S Q^T`` of ``sigma I - H``: with
        ``H = H0 + W``, ``H0 = sum_d I (x) (T_d + diag(v_d)) (x) I`` the separable part, ``T_d + diag(v_d) = Q_d
        diag(lam_d) Q_d^T`` decomposed once on the host, ``Q = Q_1 (x) ... (x) Q_D`` and
        ``S = diag(1 / max(|sigma - Lam_r|, floor * max |sigma - Lam|))``, ``Lam_r = sum_d lam_d[i_d]``.  Symmetric
        positive definite.  ``potentials``: ``None`` for the additive least-squares fit of the operator's ``V``
        (``precond_minres.separable_fit_host``), or one 1-D array per mode.  ``bases`` and ``eigenvalues``, given together,
        are used in place of a decomposition.  The decompositions are kept per potentials, ``sinv`` per ``(sigma, floor)``:
        a Lanczos run builds both once.  Returns a ``SeparablePreconditioner``."""
        tables = self._separable_tables(potentials, bases, eigenvalues)
        key = (float(sigma), float(floor))
        got = tables.by_shift.get(key)
        if got is None:
            got = tables.by_shift[key] = SeparablePreconditioner(tables, *key)
            while len(tables.by_shift) > 2:                  # the latest shifts only: each holds a vector of N doubles
                tables.by_shift.pop(next(iter(tables.by_shift)))
        return got

    @staticmethod
    def explicit_matrix(factors, diag=None):
        """The same matrix as host CSR: ``((K_1 + K_2) + ...) + diag(V)`` with ``K_d = I (x) T_d (x) I``
        (``scipy.sparse.kron``) - for checks and small problems.  Needs no device."""
        import scipy.sparse as sp
        dims = [int(np.shape(T)[0]) for T in factors]
        H = None
        for d, T in enumerate(factors):
            o = int(np.prod(dims[:d], dtype=np.int64))
            s = int(np.prod(dims[d + 1:], dtype=np.int64))
            K = sp.kron(sp.kron(sp.identity(o, format="csr"), sp.csr_matrix(np.asarray(T, dtype=np.float64)), format="csr"),
                        sp.identity(s, format="csr"), format="csr")
            H = K if H is None else H + K
        if diag is not None:
            H = H + sp.diags(np.asarray(diag, dtype=np.float64).reshape(-1), format="csr")
        return sp.csr_matrix(H)

    def to_scipy(self):
        return self.explicit_matrix(self._factors, self._diag)

    # ---- block forms: loops over single products, or refusals ---------------------------------------------------------
    def apply_block(self, xs):
        """``[H x for x in xs]``, one single product after the other."""
        ys = [self.ctx.alloc(self.nrows) for _ in xs]
        for x, y in zip(xs, ys):
            self.apply(x, y)
        return ys

    def _no_block(self, what):
        raise NotImplementedError(f"{what} needs block sweeps, which HipKronSumOperator does not have: its products and "
                                  "solves run vector by vector")

    def apply_shifted_block(self, sigma, xs, reverse=False):
        self._no_block("apply_shifted_block")

    def apply_shifted_pairs(self, z, xs, reverse=False):
        self._no_block("apply_shifted_pairs")

    def apply_shifted_block_m(self, sigma, minv, xs, reverse=False):
        self._no_block("apply_shifted_block_m")

    def apply_shifted_pairs_m(self, zs, minvs, xs, reverse=False):
        """One operand: the scaling and the single pair product (the preconditioned complex GCROT solve); more need block
        sweeps."""
        if len(xs) != 1:
            self._no_block("apply_shifted_pairs_m on several operands")
        z = np.asarray(zs, dtype=np.complex128).reshape(-1)[0]
        t = self.diag_mul(minvs[0], xs[0])
        y = (self.ctx.alloc(self.nrows), self.ctx.alloc(self.nrows))
        self.apply_shifted_pair(z, t[0], t[1], y[0], y[1], reverse=reverse)
        return [y]

    def set_variant(self, variant):
        self._no_block("set_variant (the CSR layouts)")

    def set_block_variant(self, variant):
        self._no_block("set_block_variant")

    def set_reproducible(self, on=True):
        self._no_block("set_reproducible (a choice among the CSR kernels; this product is bitwise reproducible as it is)")

    def set_reduction(self, mode):
        self._no_block("set_reduction (a choice among the CSR kernels; this product is bitwise reproducible as it is)")

    def honour_reduction_option(self, options):
        """``options["reduction"]`` is validated and met as it stands: the product has one kernel order, fixed by the dims."""
        want = (options or {}).get("reduction")
        if want not in (None, "deterministic", "fast"):
            raise ValueError(f'options["reduction"] must be "deterministic" or "fast", got {want!r}')


class _SeparableTables:
    """One decomposition on the device: the handle of ``hipeig_kron_precond_create`` with the host arrays it was built
    from.  Holds the operator: its raw-sum buffer is the scratch of an apply."""

    def __init__(self, H, handle, bases, eigenvalues):
        self.H = H
        self.ctx = H.ctx
        self.handle = handle
        self.bases = bases
        self.eigenvalues = eigenvalues
        self.by_shift = {}
        self._finalizer = weakref.finalize(self, _SeparableTables._destroy, H.ctx, handle)

    @staticmethod
    def _destroy(ctx, handle):
        _lib.load().hipeig_kron_precond_destroy(ctx.handle, handle)

    def info(self):
        out = (C.c_int64 * 40)()
        _lib.call("hipeig_kron_precond_info", self.handle, out)
        return out


class SeparablePreconditioner:
    """``M^-1 = Q S Q^T`` of ``HipKronSumOperator.separable_preconditioner`` for one shift and floor.  ``bases`` and
    ``eigenvalues`` are the host arrays ``Q_d`` and ``lam_d``; everything else runs on the device."""

    def __init__(self, tables, sigma, floor):
        self._tables = tables
        self.sigma, self.floor = sigma, floor
        self.handle = tables.handle
        self.ctx = tables.ctx
        self.bases = tables.bases
        self.eigenvalues = tables.eigenvalues
        self._sinv = None

    @property
    def n(self):
        return int(self._tables.info()[1])

    @property
    def launches_per_apply(self):
        """``2 D``: the scale rides on the last forward mode."""
        return int(self._tables.info()[2])

    @property
    def device_bytes(self):
        """The padded tables and, once built, ``sinv``.  An apply works in the operator's raw-sum buffer and in its
        output, so it owns no vector."""
        return int(self._tables.info()[3]) + (0 if self._sinv is None else 8 * self.n)

    def kernels(self):
        """Per mode the form of its transform, named as in ``HipKronSumOperator.kron_info``."""
        out = self._tables.info()
        return [HipKronSumOperator.KERNEL_FORMS[int(out[8 + 4 * d])] for d in range(int(out[0]))]

    def sinv(self):
        """Device buffer with the diagonal of ``S``; built on first use.  ``ValueError`` where an element would not be
        finite (``Lam_r == sigma`` with ``floor = 0``)."""
        if self._sinv is None:
            buf = self.ctx.alloc(self.n)
            try:
                _lib.call("hipeig_kron_precond_scale", self.ctx.handle, self.handle, self.sigma, self.floor, buf.ptr)
            except _lib.HipEigError as exc:
                if "not finite" in str(exc):
                    raise ValueError(str(exc)) from None
                raise
            self._sinv = buf
        return self._sinv

    def transform(self, d, transpose, x):
        """One mode alone (``d`` 0-based): a new device buffer with ``(I (x) Q_d (x) I) x``, ``transpose``: ``Q_d^T``."""
        if not 0 <= int(d) < len(self.bases):
            raise ValueError(f"mode {d} of {len(self.bases)}")
        z = self.ctx.alloc(self.n)
        _lib.call("hipeig_kron_precond_transform", self.ctx.handle, self.handle, int(d), 1 if transpose else 0, x.ptr, z.ptr)
        return z

    def apply(self, x):
        """A new device buffer with ``M^-1 x``."""
        z = self.ctx.alloc(self.n)
        _lib.call("hipeig_kron_precond_apply", self.ctx.handle, self.handle, self.sinv().ptr, x.ptr, z.ptr)
        return z


class HipVector(AbstractVector):
    """Device-resident fp64 vector with the NumpyVector interface.  A complex array gives a
    ``HipComplexVector`` (two real halves), the counterpart of a complex-dtype NumpyVector."""

    def __new__(cls, array=None, options=None, ctx=None):
        if cls is HipVector and not isinstance(array, DeviceBuffer) and np.iscomplexobj(array):
            return HipComplexVector(array, options, ctx=ctx)
        return super().__new__(cls)

    def __init__(self, array, options=None, ctx=None):
        given = {} if options is None else options
        if isinstance(array, DeviceBuffer):
            self._buf = array
            self.ctx = array.ctx
        else:
            host = np.ascontiguousarray(array, dtype=np.float64)
            if host.ndim != 1:
                raise ValueError("HipVector holds 1-D vectors")
            if np.iscomplexobj(array):               # only reachable from a subclass: HipVector(...) itself dispatches
                raise TypeError("a real HipVector cannot hold complex data; use HipComplexVector")
            self.ctx = ctx or HipContext.default()
            self._buf = self.ctx.alloc(host.size)
            _lib.call("hipeig_vec_upload", self.ctx.handle, self._buf.ptr,
                      host.ctypes.data_as(C.c_void_p), host.size)
        self.size = self._buf.n
        self.shape = (self._buf.n,)
        # numpyVector.py:29-36: defaults are written back into the caller's dict, which all
        # vectors derived from this one then share
        lsa = given.get("linearSystemArgs", dict())
        lsa.setdefault("linearSolver", "minres")
        lsa.setdefault("linearIter", 1000)
        lsa.setdefault("linear_tol", 1e-4)
        lsa.setdefault("linear_atol", 1e-4)
        self.options = {"linearSystemArgs": lsa}
        for extra in ("orthogonalization", "blockSolve", "reduction", "contourPoolWidth", "lanczosBasis", "lanczosBasisBytes",
                      "lanczosBasisPrefix", "lanczosBasisPrecision"):
            if extra in given:
                self.options[extra] = given[extra]
        self.last_solve_stats = None

    # ---- helpers -------------------------------------------------------------------
    def _new(self, buf):
        return HipVector(buf, self.options)

    @staticmethod
    def fromArray(template, array):
        """A vector like ``template`` (same context, shared options) from host data - the hook
        ``checkpoint.restore_vectors`` uses."""
        return HipVector(array, template.options, ctx=template.ctx)

    @property
    def array(self):
        """Host copy of the (local) data - the reference's tests read ``.array``."""
        out = np.empty(self._buf.n, dtype=np.float64)
        _lib.call("hipeig_vec_download", self.ctx.handle, out.ctypes.data_as(C.c_void_p),
                  self._buf.ptr, self._buf.n)
        return out

    # ---- properties ----------------------------------------------------------------
    @property
    def hasExactAddition(self):
        return True

    @property
    def dtype(self):
        return np.dtype(np.float64)

    @property
    def maxD(self):
        return 0

    # ---- arithmetic (out of place, numpyVector.py:57-64) ----------------------------
    def _scaled(self, alpha):
        if isinstance(alpha, complex) or np.iscomplexobj(alpha):
            alpha = complex(alpha)                      # feast.py:91-92: mult * Qe with complex mult
            return HipComplexVector(self._scaled(alpha.real), self._scaled(alpha.imag))
        out = self.ctx.alloc(self._buf.n)
        _lib.call("hipeig_scale", self.ctx.handle, self._buf.n, float(alpha), self._buf.ptr, out.ptr)
        return self._new(out)

    def __mul__(self, other):
        return self._scaled(other)

    def __rmul__(self, other):
        return self._scaled(other)

    def __truediv__(self, other):
        out = self.ctx.alloc(self._buf.n)
        _lib.call("hipeig_divide", self.ctx.handle, self._buf.n, float(other), self._buf.ptr, out.ptr)
        return self._new(out)

    def __imul__(self, other):
        raise NotImplementedError          # numpyVector.py:66-67

    def __itruediv__(self, other):
        raise NotImplementedError          # numpyVector.py:69-70

    def __len__(self):
        return self._buf.n

    # ---- instance methods -----------------------------------------------------------
    def normalize(self):
        nrm = C.c_double()
        _lib.call("hipeig_normalize", self.ctx.handle, self._buf.n, self._buf.ptr, C.byref(nrm))
        return self

    def norm(self):
        out = C.c_double()
        _lib.call("hipeig_nrm2", self.ctx.handle, self._buf.n, self._buf.ptr, C.byref(out))
        return float(out.value)

    def real(self):
        # the FEAST driver calls ``typeClass.real(mult * Qe)`` unbound, with a complex operand
        if isinstance(self, HipComplexVector):
            return self.re.copy()
        return self.copy()

    def conjugate(self):
        if isinstance(self, HipComplexVector):
            return HipComplexVector(self.re.copy(), self.im * -1.0)
        return self.copy()

    def vdot(self, other, conjugate=True):
        out = C.c_double()
        _lib.call("hipeig_dot", self.ctx.handle, self._buf.n, self._buf.ptr, other._buf.ptr, C.byref(out))
        return float(out.value)

    def copy(self):
        out = self.ctx.alloc(self._buf.n)
        _lib.call("hipeig_vec_copy", self.ctx.handle, out.ptr, self._buf.ptr, self._buf.n)
        return self._new(out)

    def applyOp(self, other):
        if not isinstance(other, HipCsrOperator):
            raise TypeError("HipVector.applyOp needs a HipCsrOperator (device-resident CSR)")
        other.honour_reduction_option(self.options)
        out = self.ctx.alloc(other.nrows)
        other.apply(self._buf, out)
        return self._new(out)

    def compress(self):
        return self

    # ---- static hooks ----------------------------------------------------------------
    @staticmethod
    def linearCombination(vectors, coeffs):
        assert len(vectors) == len(coeffs)
        v0 = vectors[0]
        cf = np.ascontiguousarray(coeffs, dtype=np.float64)
        out = v0.ctx.alloc(v0._buf.n)
        tab, keep = _ptr_table([v._buf for v in vectors])
        _lib.call("hipeig_lincomb", v0.ctx.handle, v0._buf.n, len(vectors),
                  cf.ctypes.data_as(C.POINTER(C.c_double)), tab, out.ptr)
        return v0._new(out)

    @staticmethod
    def linearCombinationBlock(vectors, coeffs):
        """k combinations at once: out[c] = sum_j coeffs[j, c] * vectors[j]
        (basisTransformation with a coefficient matrix, util_funcs.py:229-230)."""
        v0 = vectors[0]
        cm = np.ascontiguousarray(coeffs, dtype=np.float64)
        m, k = cm.shape
        assert m == len(vectors)
        outs = [v0.ctx.alloc(v0._buf.n) for _ in range(k)]
        tab, keep = _ptr_table([v._buf for v in vectors])
        otab, okeep = _ptr_table(outs)
        _lib.call("hipeig_lincomb_block", v0.ctx.handle, v0._buf.n, m, k,
                  cm.ctypes.data_as(C.POINTER(C.c_double)), k, tab, otab)
        return [v0._new(o) for o in outs]

    @staticmethod
    def orthogonalize_against_set(x, qs, lindep=LINDEP_DEFAULT_VALUE):
        """numpyVector.py:121-145.  Default: the reference's own sweep - sequential modified Gram-Schmidt
        with the division by q.q, ``None`` when what is left has x.x <= lindep - so the linear-dependency
        exit fires where the reference's does.  ``options["orthogonalization"] = "cgs2"`` selects two
        batched classical passes instead (one reduction per pass; its second pass changes the inner
        product compared with ``lindep``, so that exit may fire at another iteration)."""
        new = x.copy()
        method = _ORTHO_METHODS[x.options.get("orthogonalization", "mgs")]
        ip = C.c_double()
        dep = C.c_int()
        tab, keep = _ptr_table([q._buf for q in qs]) if len(qs) else (None, None)
        _lib.call("hipeig_orthonormalize", x.ctx.handle, new._buf.n, len(qs), tab, new._buf.ptr,
                  float(lindep), method, C.byref(ip), C.byref(dep))
        return None if dep.value else new

    @staticmethod
    def solve(H, b, sigma, x0=None, opType="her", reverseGF=False):
        """``(sigma I - H) x = b`` (``reverseGF``: ``(H - sigma I) x = b``) with the solver and limits of
        ``b.options["linearSystemArgs"]`` (numpyVector.py:147-178); ``UserWarning`` on non-convergence.

        ``linearSystemArgs["preconditioner"] = "jacobi"`` (default ``None``; with ``linearSolver="minres"``, a real shift,
        no ``x0``, one GPU - anything else raises) runs SciPy's ``minres(A, b, M=...)`` with the diagonal
        ``M = diag(max(|sigma - h_ii|, f * max_j |sigma - h_jj|))``, ``f = linearSystemArgs["preconditionerFloor"]``
        (relative, ``>= 0``, default 1e-8: only a guard against ``h_ii == sigma``; ``f = 0`` with an exact hit raises
        ``ValueError``).  ``reverseGF`` flips the sign only, ``M`` is the same.  ``linear_tol`` is then tested in SciPy's
        PRECONDITIONED quantities - ``beta1 = sqrt(<b, M^-1 b>)`` and the residual estimate ``phibar`` in the ``M^-1`` norm,
        exactly what ``scipy.sparse.linalg.minres(A, b, M=...)`` does - so the 2-norm residual at the stop is not the plain
        solve's.  ``last_solve_stats`` keeps its keys and gains ``"preconditioner": "jacobi"``.  It pays on diagonally
        dominant operators and buys nothing on others.

        ``linearSystemArgs["preconditioner"] = "separable"`` (same conditions, and ``H`` a ``HipKronSumOperator`` -
        ``NotImplementedError`` otherwise) runs the same SciPy solve with the fast-diagonalisation
        ``M^-1 = Q S Q^T`` of ``H.separable_preconditioner``: the separable part of ``H``, the factors
        plus 1-D potentials, inverted exactly.  ``linearSystemArgs["preconditionerPotentials"]`` is ``None`` (the additive
        least-squares fit of the operator's ``V``) or a list of one 1-D array per mode; ``"preconditionerFloor"`` means what
        it means for Jacobi.  ``last_solve_stats`` gains ``"preconditioner": "separable"``.

        ``linearSystemArgs["gcrotPreconditioner"] = "jacobi"`` (default ``None``; with ``linearSolver="gcrotmk"``, no
        ``x0``, one GPU, a whole operator - anything else raises) is the key of the GCROT solves, real shift or complex
        contour point ``z``, here and in every lock-step form of ``solveBlock``: SciPy's ``gcrotmk(A, b, M=...)`` with the
        diagonal ``M = diag(1 / (z - h_ii))``, kept away from ``h_ii == z`` by the same relative
        ``"preconditionerFloor"`` (``HipCsrOperator.jacobi_inverse_z``).  SciPy applies ``M`` on the right, so the
        unchanged solver runs on ``sign (z I - H) M`` and its result ``u`` is returned as ``x = M u``; the residual it
        tests is the true one, so ``linear_tol`` and ``linear_atol`` keep their meaning.  ``last_solve_stats`` gains
        ``"preconditioner": "jacobi"``.  DESIGN.md 3.4b says where it pays and where it does not."""
        if not isinstance(H, HipCsrOperator):
            raise TypeError("HipVector.solve needs a HipCsrOperator (device-resident CSR)")
        pre = _preconditioner(b.options["linearSystemArgs"], sigma, x0, b.ctx, H)
        gfloor = _gcrot_preconditioner(b.options["linearSystemArgs"], x0, b.ctx, H)
        if isinstance(b, HipComplexVector):                 # HipVector(complex array) is a HipComplexVector: same entry point
            return HipComplexVector.solve(H, b, sigma, x0, opType, reverseGF)
        if b.options["linearSystemArgs"]["linearSolver"] == "minres_shifted":
            # one-shift call of the shared-Lanczos solver (shifted_minres.solve_shifts): a HipComplexVector for a real shift too
            if x0 is not None:
                raise NotImplementedError("linearSolver='minres_shifted' starts from x = 0 (no initial guess)")
            return HipVector._solve_shifts(H, b, [sigma], reverseGF)[0]
        if b.options["linearSystemArgs"]["linearSolver"] == "lanczos_filter":
            raise NotImplementedError("linearSolver='lanczos_filter' returns FEAST's filtered sums, not solutions: use "
                                      "feastDiagonalization or lanczos_filter.lanczos_filter")
        if x0 is not None and not isinstance(x0, (HipVector, HipComplexVector)):
            x0 = HipVector(np.asarray(x0), ctx=b.ctx)      # NumpyVector hands an ndarray on to SciPy; complex arrays become HipComplexVector
        if isinstance(x0, HipComplexVector) and not (isinstance(sigma, complex) or np.iscomplexobj(sigma)):
            return HipComplexVector.solve(H, HipComplexVector(b, b * 0.0), sigma, x0, opType, reverseGF)    # a complex guess makes the solve complex
        H.honour_reduction_option(b.options)
        o = b.options["linearSystemArgs"]
        name = o["linearSolver"]
        if name == "pardiso":
            return HipVector._solve_exact_small(H, b, sigma, reverseGF)
        if isinstance(sigma, complex) or np.iscomplexobj(sigma):
            return HipVector._solve_complex(H, b, complex(sigma), o, reverseGF, x0)
        if name == "gcrotmk":
            # numpyVector.py:161: gcrotmk(linOp, b, x0, tol, atol, maxiter) with SciPy's m = k = 20
            from .gcrotmk import gcrotmk_device
            minv = None if gfloor is None else H.jacobi_inverse_z(float(sigma), gfloor)

            def matvec(buf):
                out = b.ctx.alloc(b._buf.n)
                if minv is not None:                        # SciPy's right preconditioner: w = A (M v)
                    H.apply_shifted_m(sigma, minv, buf, out, reverse=reverseGF)
                else:
                    H.apply_shifted(sigma, buf, out, reverse=reverseGF)
                return out

            xbuf, conv, gstats = gcrotmk_device(b.ctx, matvec, b._buf, b._buf.n, rtol=float(o["linear_tol"]),
                                                atol=float(o["linear_atol"]), maxiter=int(o["linearIter"]),
                                                x0=None if x0 is None else x0._buf,
                                                cols_per_pass=int(o.get("arnoldiColumnsPerPass", 1)))
            if minv is not None:
                H.diag_mul(minv, xbuf, xbuf)                # x = M u
            res = b._new(xbuf)
            res.last_solve_stats = b.last_solve_stats = {"iterations": gstats["matvecs"], "outer": gstats["outer"]}
            if minv is not None:
                res.last_solve_stats["preconditioner"] = "jacobi"
            if conv != 0:
                raise UserWarning("Warning:: Iterative solver is not converged ")
            return res
        if name != "minres":
            raise Exception("Got linear solver other than gcrotmk, minres and pardiso!")
        out = b.ctx.alloc(b._buf.n)
        info = C.c_int()
        stats = (C.c_double * 8)()
        if pre == "jacobi":
            minv = H.jacobi_inverse(float(sigma), float(o.get("preconditionerFloor", PRECONDITIONER_FLOOR_DEFAULT)))
            _lib.call("hipeig_minres_jacobi", b.ctx.handle, H.handle, float(sigma), -1.0 if reverseGF else 1.0,
                      b._buf.ptr, minv.ptr, out.ptr, float(o["linear_tol"]), int(o["linearIter"]), C.byref(info), stats)
        elif pre == "separable":
            P = H.separable_preconditioner(float(sigma), float(o.get("preconditionerFloor", PRECONDITIONER_FLOOR_DEFAULT)),
                                           potentials=o.get("preconditionerPotentials"))
            _lib.call("hipeig_minres_kron_separable", b.ctx.handle, H.handle, P.handle, P.sinv().ptr, float(sigma),
                      -1.0 if reverseGF else 1.0, b._buf.ptr, out.ptr, float(o["linear_tol"]), int(o["linearIter"]),
                      C.byref(info), stats)
        elif x0 is None:
            _lib.call("hipeig_minres", b.ctx.handle, H.handle, float(sigma), -1.0 if reverseGF else 1.0,
                      b._buf.ptr, out.ptr, float(o["linear_tol"]), int(o["linearIter"]), C.byref(info), stats)
        else:               # scipy.sparse.linalg.minres(linOp, b, x0): r1 = b - A x0, the iterate starts at x0
            _lib.call("hipeig_minres_x0", b.ctx.handle, H.handle, float(sigma), -1.0 if reverseGF else 1.0,
                      b._buf.ptr, x0._buf.ptr, out.ptr, float(o["linear_tol"]), int(o["linearIter"]), C.byref(info), stats)
        res = b._new(out)
        res.last_solve_stats = {"iterations": int(stats[0]), "istop": int(stats[1]), "rnorm": stats[2],
                                "Anorm": stats[3], "ynorm": stats[4], "test1": stats[5],
                                "test2": stats[6], "Acond": stats[7]}
        if pre is not None:
            res.last_solve_stats["preconditioner"] = pre
        if b.ctx.nranks > 1 or os.environ.get("HIPEIG_FORCE_COLLECTIVES", "0") not in ("", "0"):
            cs = (C.c_int64 * 4)()
            _lib.call("hipeig_comm_stats", b.ctx.handle, cs)
            res.last_solve_stats["collectives"] = int(cs[0])
        b.last_solve_stats = res.last_solve_stats
        if info.value != 0:
            # numpyVector.py:175-177: the warning is escalated to an exception
            raise UserWarning("Warning:: Iterative solver is not converged ")
        return res

    @staticmethod
    def _solve_shifts(H, b, shifts, reverseGF=False):
        """All of ``shifts`` for one right-hand side from one Lanczos run (``shifted_minres.solve_shifts``); the hook
        ``feastDiagonalization`` looks for when ``linearSolver`` is ``"minres_shifted"``."""
        from .shifted_minres import solve_shifts
        _preconditioner(b.options["linearSystemArgs"])
        return solve_shifts(H, b, shifts, reverseGF=reverseGF)

    @staticmethod
    def _lanczos_filter(H, B, shifts, weights, reverseGF=False):
        """``sum_j Re(weights[j] x_j)`` for every right-hand side of ``B`` from two Lanczos passes, no solution formed
        (``lanczos_filter.lanczos_filter``); the hook ``feastDiagonalization`` looks for when ``linearSolver`` is
        ``"lanczos_filter"``.  ``B[0].options["lanczosBasis"]`` (``"recompute"``, the default, or ``"keep"``) and
        ``["lanczosBasisBytes"]`` choose whether pass 1 keeps its vectors for pass 2 and the byte budget of that;
        ``["lanczosBasisPrefix"]: True`` (only with ``"keep"``, ``ValueError`` otherwise) lets a basis that outgrows the
        budget keep the vectors that fit; ``["lanczosBasisPrecision"]: "fp32"`` (only with ``"keep"`` too) stores the basis
        in fp32."""
        from .lanczos_filter import lanczos_filter
        _need_block_sweeps(H, 'linearSolver="lanczos_filter"')
        B = list(B)
        o = B[0].options if B else {}
        if B:
            _preconditioner(o["linearSystemArgs"])
        if o.get("lanczosBasisPrefix") and o.get("lanczosBasis", "recompute") != "keep":
            raise ValueError('"lanczosBasisPrefix" keeps a prefix of a kept basis: it needs "lanczosBasis": "keep"')
        if o.get("lanczosBasisPrecision", "fp64") == "fp32" and o.get("lanczosBasis", "recompute") != "keep":
            raise ValueError('"lanczosBasisPrecision": "fp32" stores a kept basis in fp32: it needs "lanczosBasis": "keep"')
        return lanczos_filter(H, B, shifts, weights, reverseGF=reverseGF, basis=o.get("lanczosBasis", "recompute"),
                              basisBytes=o.get("lanczosBasisBytes"), prefix=bool(o.get("lanczosBasisPrefix", False)),
                              precision=o.get("lanczosBasisPrecision", "fp64"))

    BLOCK_SOLVE_MIN = 3      # fewer right-hand sides are solved one by one (measured at N = 1e6: 2 columns 0.97x, 3: 1.6x, 4: 1.95x, 8: 2.8x)

    @staticmethod
    def solveBlock(H, bs, sigma, x0=None, opType="her", reverseGF=False, onSolution=None, poolStats=None):
        """``[solve(H, b, sigma) for b in bs]`` with the solves advanced in lock step: one block product
        per MINRES iteration for up to 8 right-hand sides (inexact_Lanczos.py:319-320 calls ``solve``
        once per block vector on the same operator and shift).  Every column runs the recurrences and
        stopping tests of the single solve; results, ``last_solve_stats`` and the exception on
        non-convergence (numpyVector.py:175-177) are those of the one-by-one calls.  Blocks of <= 4 use a
        4-wide interleave (twice the rows per workgroup), larger ones chunks of 8.  GCROT runs its solves in lock step
        too, for a complex shift (``_solve_complex_block``) and for a real one from ``BLOCK_SOLVE_MIN_GCROT`` right-hand
        sides on, ``BLOCK_SOLVE_MIN_GCROT_LONG`` for vectors longer than one Arnoldi batch (n > 8192;
        ``_solve_real_block``; not with ``options["blockSolve"] = False``).  A context with collectives solves one by one.  Other solvers, an initial guess
        and fewer right-hand sides take the one-by-one calls.

        ``sigma`` may also be a sequence of ``len(bs)`` shifts, one per right-hand side: the solves of all contour points
        of a FEAST iteration are independent (feast.py:189-200).  Complex shifts with GCROT, no ``x0``, on one GPU without
        collectives run as an always-full pool of lock-step solves (``_solve_complex_pool``); anything else one by one,
        each with its shift.  ``onSolution(i, x_i)``, when given, is called the moment solve i has ended (in the order
        the solves end) and the returned list then holds ``None`` in place of the solutions handed out, so that a caller
        who folds each solution into a sum never holds all of them.  ``poolStats``, a dict, receives the pool's record
        (width, rounds, block products by live operands, products and outer iterations per solve) when the pool ran.

        With ``linearSystemArgs["preconditioner"]`` set the solves are the one-by-one ``solve`` calls whatever the block
        size, unless ``linearSystemArgs["preconditionerLockStep"]`` is ``True`` (default ``False``; a ``bool``, and only with
        ``"preconditioner": "jacobi"`` - anything else raises ``ValueError``).  Then one real shift, no ``x0``, at least
        ``BLOCK_SOLVE_MIN`` right-hand sides, a ``HipCsrOperator`` and a context without collectives run the lock-step
        block form of the preconditioned solve (``hipeig_minres_block_jacobi``) in chunks of 8, the 4-wide
        interleave for 4 or fewer: every column runs the recurrence and stopping tests of the preconditioned single solve,
        ``M`` is the single solve's (``H.jacobi_inverse``), and ``last_solve_stats`` gains ``"preconditioner": "jacobi"``
        and ``"lockStep": True``.  A block product adds a row in another order than the single sweep, so the results agree
        with the one-by-one solves to the solve tolerance, not bit for bit; every other case takes the one-by-one calls
        with their refusals."""
        bs = list(bs)
        if bs and _preconditioner(bs[0].options["linearSystemArgs"]) is not None:
            o = bs[0].options["linearSystemArgs"]
            if (o.get("preconditionerLockStep", False) and np.ndim(sigma) == 0
                    and not (isinstance(sigma, complex) or np.iscomplexobj(sigma)) and x0 is None
                    and len(bs) >= HipVector.BLOCK_SOLVE_MIN and isinstance(H, HipCsrOperator)
                    and all(isinstance(b, HipVector) for b in bs)
                    and not bs[0].ctx.collectives and not bs[0].ctx.direct_only):
                _need_block_sweeps(H, '"preconditionerLockStep": True')
                sols = HipVector._solve_block_minres(H, bs, float(sigma), o, reverseGF, jacobi=True)
                if onSolution is not None:
                    for i, xs in enumerate(sols):
                        onSolution(i, xs)
                    return [None] * len(sols)
                return sols
            # one by one whatever the block size: every refusal and result is that of solve()
            shifts = list(sigma) if np.ndim(sigma) > 0 else [sigma] * len(bs)
            if len(shifts) != len(bs):
                raise ValueError(f"{len(shifts)} shifts for {len(bs)} right-hand sides")
            out = []
            for i, (b, z) in enumerate(zip(bs, shifts)):
                xs = HipVector.solve(H, b, z, x0, opType, reverseGF)
                if onSolution is not None:
                    onSolution(i, xs)
                    xs = None
                out.append(xs)
            return out
        if np.ndim(sigma) > 0:
            return HipVector._solve_block_shifts(H, bs, list(sigma), x0, opType, reverseGF, onSolution, poolStats)
        if onSolution is not None:
            sols = HipVector.solveBlock(H, bs, sigma, x0, opType, reverseGF)
            for i, x in enumerate(sols):
                onSolution(i, x)
            return [None] * len(sols)
        o = bs[0].options["linearSystemArgs"]
        complex_shift = isinstance(sigma, complex) or np.iscomplexobj(sigma)

        def whole():
            # whole vectors on a context without collectives (one GPU, or FEAST's contour replicas): the split Arnoldi steps
            # run on one GPU only; a row partition - or one rank rehearsing it with HIPEIG_FORCE_COLLECTIVES - solves one by one
            return (isinstance(H, HipCsrOperator) and H.supports_block_sweeps and not bs[0].ctx.direct_only
                    and not bs[0].ctx.collectives and all(isinstance(b, HipVector) for b in bs))

        if o["linearSolver"] == "gcrotmk" and complex_shift and x0 is None and len(bs) >= 2 and whole():
            return HipVector._solve_complex_block(H, bs, complex(sigma), o, reverseGF)
        if (o["linearSolver"] == "gcrotmk" and not complex_shift and x0 is None and bs[0].options.get("blockSolve", True)
                and whole()):
            from .gcrotmk import _Ops
            if len(bs) >= (BLOCK_SOLVE_MIN_GCROT if len(bs[0]) <= _Ops.BATCH_MAX_N else BLOCK_SOLVE_MIN_GCROT_LONG):
                return HipVector._solve_real_block(H, bs, float(sigma), o, reverseGF)
        if (o["linearSolver"] != "minres" or isinstance(sigma, complex) or np.iscomplexobj(sigma)
                or x0 is not None or len(bs) < HipVector.BLOCK_SOLVE_MIN or not isinstance(H, HipCsrOperator)
                or not H.supports_block_sweeps or bs[0].ctx.direct_only):
            return [HipVector.solve(H, b, sigma, x0, opType, reverseGF) for b in bs]
        return HipVector._solve_block_minres(H, bs, float(sigma), o, reverseGF)

    @staticmethod
    def _solve_block_minres(H, bs, sigma, o, reverseGF, jacobi=False):
        """The lock-step MINRES solves of ``solveBlock`` in chunks of 8 right-hand sides: ``hipeig_minres_block``, or with
        ``jacobi`` its preconditioned form ``hipeig_minres_block_jacobi`` with the single solve's ``M^-1``."""
        H.honour_reduction_option(bs[0].options)
        ctx, n = bs[0].ctx, bs[0]._buf.n
        if jacobi:
            minv = H.jacobi_inverse(sigma, float(o.get("preconditionerFloor", PRECONDITIONER_FLOOR_DEFAULT)))
        results = []
        for i0 in range(0, len(bs), 8):
            chunk = bs[i0:i0 + 8]
            k = len(chunk)
            outs = [ctx.alloc(n) for _ in chunk]
            bt, keep1 = _ptr_table([b._buf for b in chunk])
            xt, keep2 = _ptr_table(outs)
            info = (C.c_int * k)()
            stats = (C.c_double * (8 * k))()
            if jacobi:
                _lib.call("hipeig_minres_block_jacobi", ctx.handle, H.handle, sigma, -1.0 if reverseGF else 1.0, k,
                          bt, minv.ptr, xt, float(o["linear_tol"]), int(o["linearIter"]), info, stats)
            else:
                _lib.call("hipeig_minres_block", ctx.handle, H.handle, sigma, -1.0 if reverseGF else 1.0, k,
                          bt, xt, float(o["linear_tol"]), int(o["linearIter"]), info, stats)
            ncoll = None
            if ctx.nranks > 1 or os.environ.get("HIPEIG_FORCE_COLLECTIVES", "0") not in ("", "0"):
                cs = (C.c_int64 * 4)()
                _lib.call("hipeig_comm_stats", ctx.handle, cs)
                ncoll = int(cs[0])                 # collectives of the whole lock-step solve (all columns together)
            for j, b in enumerate(chunk):
                res = b._new(outs[j])
                st = stats[8 * j:8 * j + 8]
                res.last_solve_stats = b.last_solve_stats = {
                    "iterations": int(st[0]), "istop": int(st[1]), "rnorm": st[2], "Anorm": st[3],
                    "ynorm": st[4], "test1": st[5], "test2": st[6], "Acond": st[7]}
                if ncoll is not None:
                    res.last_solve_stats["collectives"] = ncoll
                if jacobi:
                    res.last_solve_stats["preconditioner"] = "jacobi"
                    res.last_solve_stats["lockStep"] = True
                results.append(res)
            if any(info[j] != 0 for j in range(k)):
                raise UserWarning("Warning:: Iterative solver is not converged ")
        return results

    EXACT_SOLVE_MAX = 96

    @staticmethod
    def _solve_exact_small(H, b, sigma, reverseGF):
        """``linearSolver="pardiso"`` (numpyVector.py:166-170: ``spsolve`` of ``sigma*I - H``, which the reference keeps
        "only for comparing with fortran"): Gaussian elimination with partial pivoting on the device, one workgroup,
        n <= 96.  Real or complex shift, real or complex right-hand side; never a CPU detour."""
        ctx, n = b.ctx, len(b)
        if n > HipVector.EXACT_SOLVE_MAX:
            raise NotImplementedError(f"linearSolver='pardiso' is the reference's small exact branch (Fortran comparison); "
                                      f"on the device it takes n <= {HipVector.EXACT_SOLVE_MAX}, got n = {n}")
        z = complex(sigma)
        cplx_b = isinstance(b, HipComplexVector)
        br = b.re if cplx_b else b
        bi = b.im._buf.ptr if cplx_b else None
        is_complex = cplx_b or z.imag != 0.0 or isinstance(sigma, complex) or np.iscomplexobj(sigma)
        xr = ctx.alloc(n)
        xi = ctx.alloc(n) if is_complex else None
        flag = C.c_int()
        _lib.call("hipeig_dense_solve_small", ctx.handle, H.handle, z.real, z.imag, -1.0 if reverseGF else 1.0,
                  br._buf.ptr, bi, xr.ptr, None if xi is None else xi.ptr, C.byref(flag))
        if flag.value:
            raise np.linalg.LinAlgError("sigma*I - H is singular to working precision")
        res = HipComplexVector(br._new(xr), br._new(xi)) if is_complex else br._new(xr)
        res.last_solve_stats = b.last_solve_stats = {"iterations": 0, "exact": True}
        return res

    @staticmethod
    def _solve_complex(H, b, z, o, reverseGF, x0=None):
        """(z*I - H) x = b with a complex contour point z, real H and real b (feast.py:83-90).
        The system is complex symmetric, so the reference uses GCROT there; the complex vectors
        are (re, im) pairs of device buffers and one complex product costs two operator sweeps."""
        if o["linearSolver"] != "gcrotmk":
            raise NotImplementedError("complex shifts need linearSolver='gcrotmk' on the device "
                                      f"(got {o['linearSolver']!r}; minres is for Hermitian systems)")
        from .gcrotmk import gcrotmk_device
        ctx, n = b.ctx, len(b)
        sgn = -1.0 if reverseGF else 1.0
        gfloor = _gcrot_preconditioner(o, x0, ctx, H)
        minv = None if gfloor is None else H.jacobi_inverse_z(z, gfloor)

        def matvec(v):                                  # sgn * ((zr + i zi)(vr + i vi) - H vr - i H vi)
            if minv is not None:                        # SciPy's right preconditioner: w = A (M v)
                return H.apply_shifted_pairs_m([z], [minv], [v], reverse=reverseGF)[0]
            out_r, out_i = ctx.alloc(n), ctx.alloc(n)
            H.apply_shifted_pair(z, v[0], v[1], out_r, out_i, reverse=reverseGF)
            return (out_r, out_i)

        if isinstance(b, HipComplexVector):
            rhs = (b.re._buf, b.im._buf)
            b = b.re
        else:
            zero = ctx.alloc(n)
            _lib.call("hipeig_vec_fill", ctx.handle, zero.ptr, n, 0.0)
            rhs = (b._buf, zero)
        guess = None
        if x0 is not None:                              # SciPy's x0 (numpyVector.py:161): real or complex, array or vector
            if not isinstance(x0, (HipVector, HipComplexVector)):
                x0 = HipVector(np.asarray(x0), ctx=ctx)              # complex arrays come back as HipComplexVector
            if isinstance(x0, HipComplexVector):
                guess = (x0.re._buf, x0.im._buf)
            else:
                zero0 = ctx.alloc(n)
                _lib.call("hipeig_vec_fill", ctx.handle, zero0.ptr, n, 0.0)
                guess = (x0._buf, zero0)
        x, conv, gstats = gcrotmk_device(ctx, matvec, rhs, n, rtol=float(o["linear_tol"]),
                                         atol=float(o["linear_atol"]), maxiter=int(o["linearIter"]),
                                         complex_pairs=True, x0=guess,
                                         cols_per_pass=int(o.get("arnoldiColumnsPerPass", 1)))
        if minv is not None:
            H.diag_mul(minv, x, x)                      # x = M u
        res = HipComplexVector(b._new(x[0]), b._new(x[1]))
        res.last_solve_stats = b.last_solve_stats = {"iterations": gstats["matvecs"], "outer": gstats["outer"]}
        if minv is not None:
            res.last_solve_stats["preconditioner"] = "jacobi"
        if conv != 0:
            raise UserWarning("Warning:: Iterative solver is not converged ")
        return res

    @staticmethod
    def _solve_complex_block(H, bs, z, o, reverseGF):
        """The contour solves (z*I - H) x_i = b_i of ONE contour point for all right-hand sides in lock step
        (feast.py:198-200 runs them one after the other on the same operator and shift): each is the complex GCROT of
        ``_solve_complex``, unchanged, but their operator applications are collected and run as block products, four
        complex operands per pass over the operator (``gcrotmk_device_block``, ``hipeig_spmm_shift_pairs``).  Results,
        ``last_solve_stats`` and the exception on non-convergence are those of the one-by-one solves."""
        from .gcrotmk import gcrotmk_device_block
        ctx, n = bs[0].ctx, len(bs[0])
        H.honour_reduction_option(bs[0].options)
        rhs = []
        for b in bs:
            zero = ctx.alloc(n)
            _lib.call("hipeig_vec_fill", ctx.handle, zero.ptr, n, 0.0)
            rhs.append((b._buf, zero))

        gfloor = _gcrot_preconditioner(o, None, ctx, H)
        minv = None if gfloor is None else H.jacobi_inverse_z(z, gfloor)

        def block_matvec(vs):
            if minv is not None:
                return H.apply_shifted_pairs_m([z] * len(vs), [minv] * len(vs), vs, reverse=reverseGF)
            return H.apply_shifted_pairs(z, vs, reverse=reverseGF)

        sols = gcrotmk_device_block(ctx, block_matvec, rhs, n, rtol=float(o["linear_tol"]), atol=float(o["linear_atol"]),
                                    maxiter=int(o["linearIter"]), complex_pairs=True,
                                    cols_per_pass=int(o.get("arnoldiColumnsPerPass", 1)))
        out, failed = [], False
        for b, (x, conv, gstats) in zip(bs, sols):
            if minv is not None:
                H.diag_mul(minv, x, x)
            res = HipComplexVector(b._new(x[0]), b._new(x[1]))
            res.last_solve_stats = b.last_solve_stats = {"iterations": gstats["matvecs"], "outer": gstats["outer"]}
            if minv is not None:
                res.last_solve_stats["preconditioner"] = "jacobi"
            failed = failed or conv != 0
            out.append(res)
        if failed:
            raise UserWarning("Warning:: Iterative solver is not converged ")
        return out

    @staticmethod
    def _solve_block_shifts(H, bs, shifts, x0, opType, reverseGF, onSolution, poolStats):
        """``solveBlock`` with one shift per right-hand side."""
        if len(shifts) != len(bs):
            raise ValueError(f"{len(shifts)} shifts for {len(bs)} right-hand sides")
        o = bs[0].options["linearSystemArgs"]
        if (o["linearSolver"] == "gcrotmk" and x0 is None and isinstance(H, HipCsrOperator) and H.supports_block_sweeps
                and all(isinstance(z, (complex, np.complexfloating)) for z in shifts)
                and all(isinstance(b, HipVector) for b in bs)
                and not bs[0].ctx.direct_only and not bs[0].ctx.collectives):
            return HipVector._solve_complex_pool(H, bs, [complex(z) for z in shifts], o, reverseGF, onSolution, poolStats)
        out = []
        for i, (b, z) in enumerate(zip(bs, shifts)):
            x = HipVector.solve(H, b, z, x0, opType, reverseGF)
            if onSolution is not None:
                onSolution(i, x)
                x = None
            out.append(x)
        return out

    # Device memory one complex GCROT(m, k) solve keeps alive, in complex vectors (16 n bytes each): the iterate and the
    # residual (2), c outer pairs (2c) and the Arnoldi vectors of a cycle of m + (k - c) steps (m + k - c + 1), largest with
    # the recycle space full (c = k): 2k + m + 1; plus the new pair (ux, cx), the product just returned and the operand of
    # a complex scaling while they are being built (4).  SciPy's m = k = 20: 67 vectors, 1072 n bytes.  With
    # linearSystemArgs["gcrotPreconditioner"] the pool also holds one Minv per distinct contour point (16 n bytes each, the
    # HipCsrOperator.JACOBI_Z_CACHE latest stay with the operator): they belong to the call, not to a solve, and are built
    # before _pool_width reads the free memory, so its estimate has already paid for them.
    @staticmethod
    def _pool_vectors_per_solve(m=20, k=20):
        return 2 + (2 * k + m + 1) + 4

    @staticmethod
    def _pool_width(ctx, n, options):
        """Solves the contour pool keeps alive: ``options["contourPoolWidth"]`` when set, else min(16, what nine tenths of
        the free device memory - the context's recycled buffers of this length included - hold), at least 1."""
        from .gcrotmk import POOL_MAX_WIDTH
        forced = options.get("contourPoolWidth")
        if forced is not None:
            return max(1, min(POOL_MAX_WIDTH, int(forced)))
        free = ctx.device_info()["hbm_free"] + 8 * n * len(ctx._pool.get(n, ()))
        per_solve = 16 * n * HipVector._pool_vectors_per_solve()
        return max(1, min(POOL_MAX_WIDTH, int(0.9 * free) // per_solve))

    @staticmethod
    def _solve_complex_pool(H, bs, zs, o, reverseGF, onSolution, poolStats):
        """The contour solves (z_i*I - H) x_i = b_i, every right-hand side with its own contour point, through an
        always-full pool of lock-step solves (``gcrotmk_device_pool``): each is the complex GCROT of ``_solve_complex``,
        unchanged; at most ``_pool_width`` of them are alive, a slot that ends is refilled before the next block product
        (``hipeig_spmm_shift_pairs_z``: a shift per operand).  Results, ``last_solve_stats`` and the exception on
        non-convergence, raised once every solve has run, are those of the one-by-one solves.  The pool's own record goes
        into ``poolStats``."""
        from .gcrotmk import gcrotmk_device_pool
        ctx, n = bs[0].ctx, len(bs[0])
        H.honour_reduction_option(bs[0].options)
        zero = ctx.alloc(n)                              # the right-hand sides are real and only read: one zero half for all
        _lib.call("hipeig_vec_fill", ctx.handle, zero.ptr, n, 0.0)

        gfloor = _gcrot_preconditioner(o, None, ctx, H)
        # a minv per contour point, built before _pool_width reads the free memory so that its estimate sees them
        minvs = None if gfloor is None else {z: H.jacobi_inverse_z(z, gfloor) for z in dict.fromkeys(zs)}

        def block_matvec(vs, tags):
            if minvs is not None:
                return H.apply_shifted_pairs_m([zs[t] for t in tags], [minvs[zs[t]] for t in tags], vs, reverse=reverseGF)
            return H.apply_shifted_pairs([zs[t] for t in tags], vs, reverse=reverseGF)

        pool = poolStats if poolStats is not None else {}
        out, failed = [None] * len(bs), False
        for i, _, x, conv, gstats in gcrotmk_device_pool(
                ctx, block_matvec, [((b._buf, zero), i) for i, b in enumerate(bs)], n, HipVector._pool_width(ctx, n, bs[0].options),
                rtol=float(o["linear_tol"]), atol=float(o["linear_atol"]), maxiter=int(o["linearIter"]),
                complex_pairs=True, cols_per_pass=int(o.get("arnoldiColumnsPerPass", 1)), pool_stats=pool):
            b = bs[i]
            if minvs is not None:
                H.diag_mul(minvs[zs[i]], x, x)
            res = HipComplexVector(b._new(x[0]), b._new(x[1]))
            res.last_solve_stats = b.last_solve_stats = {"iterations": gstats["matvecs"], "outer": gstats["outer"]}
            if minvs is not None:
                res.last_solve_stats["preconditioner"] = "jacobi"
            failed = failed or conv != 0
            if onSolution is not None:
                onSolution(i, res)
            else:
                out[i] = res
        if failed:
            raise UserWarning("Warning:: Iterative solver is not converged ")
        return out

    @staticmethod
    def _solve_real_block(H, bs, sigma, o, reverseGF):
        """The shifted solves sign*(sigma*I - H) x_i = b_i of one block Lanczos iteration (inexact_Lanczos.py:319-320 runs
        them one after the other on the same operator and real shift) in lock step: each is the GCROT of ``solve``,
        unchanged - its own spaces, its own stopping - but their operator applications run as block products, eight
        operands per pass over the operator (``gcrotmk_device_block``, ``hipeig_spmm_shift``), and their Arnoldi steps are
        enqueued back to back (one launch for all of them at n <= 8192).  Results, ``last_solve_stats`` (plus
        ``"lock_step": True``) and the exception on non-convergence, raised once every solve has run, are those of the
        one-by-one solves."""
        from .gcrotmk import gcrotmk_device_block
        ctx, n = bs[0].ctx, bs[0]._buf.n
        H.honour_reduction_option(bs[0].options)

        gfloor = _gcrot_preconditioner(o, None, ctx, H)
        minv = None if gfloor is None else H.jacobi_inverse_z(sigma, gfloor)

        def block_matvec(vs):
            if minv is not None:
                return H.apply_shifted_block_m(sigma, minv, vs, reverse=reverseGF)
            return H.apply_shifted_block(sigma, vs, reverse=reverseGF)

        sols = gcrotmk_device_block(ctx, block_matvec, [b._buf for b in bs], n, rtol=float(o["linear_tol"]),
                                    atol=float(o["linear_atol"]), maxiter=int(o["linearIter"]),
                                    cols_per_pass=int(o.get("arnoldiColumnsPerPass", 1)))
        out, failed = [], False
        for b, (x, conv, gstats) in zip(bs, sols):
            if minv is not None:
                H.diag_mul(minv, x, x)
            res = b._new(x)
            res.last_solve_stats = b.last_solve_stats = {"iterations": gstats["matvecs"], "outer": gstats["outer"],
                                                         "lock_step": True}
            if minv is not None:
                res.last_solve_stats["preconditioner"] = "jacobi"
            failed = failed or conv != 0
            out.append(res)
        if failed:
            raise UserWarning("Warning:: Iterative solver is not converged ")
        return out

    @staticmethod
    def _multi_dot(vectors, x):
        v0 = vectors[0]
        out = np.empty(len(vectors), dtype=np.float64)
        tab, keep = _ptr_table([v._buf for v in vectors])
        _lib.call("hipeig_multi_dot", v0.ctx.handle, v0._buf.n, len(vectors), tab, x._buf.ptr,
                  out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    @staticmethod
    def overlapMatrix(vectors):
        m = len(vectors)
        v0 = vectors[0]
        S = np.empty((m, m), dtype=np.float64)
        tab, keep = _ptr_table([v._buf for v in vectors])
        _lib.call("hipeig_gram", v0.ctx.handle, v0._buf.n, m, tab, m, tab,
                  S.ctypes.data_as(C.POINTER(C.c_double)))
        return np.triu(S) + np.triu(S, 1).T            # upper triangle mirrored, numpyVector.py:199-202

    @staticmethod
    def matrixRepresentation(operator, vectors):
        if not isinstance(operator, HipCsrOperator):
            raise TypeError("HipVector.matrixRepresentation needs a HipCsrOperator (device-resident CSR)")
        m = len(vectors)
        v0 = vectors[0]
        operator.honour_reduction_option(v0.options)
        # all kets H y_j in one block product, then one Gram block <y_i, H y_j> on the matrix cores
        kets = operator.apply_block([v._buf for v in vectors])
        M = np.empty((m, m), dtype=np.float64)
        ta, keep1 = _ptr_table([v._buf for v in vectors])
        tb, keep2 = _ptr_table(kets)
        _lib.call("hipeig_gram", v0.ctx.handle, v0._buf.n, m, ta, m, tb, M.ctypes.data_as(C.POINTER(C.c_double)))
        return np.tril(M) + np.tril(M, -1).T           # lower triangle mirrored, numpyVector.py:186-189

    @staticmethod
    def extendOverlapMatrix(vectors, overlap):
        col = HipVector._multi_dot(vectors, vectors[-1])
        m = len(vectors)
        S = np.empty((m, m), dtype=np.float64)
        S[:m - 1, :m - 1] = overlap
        S[:, m - 1] = col
        S[m - 1, :] = col
        return S

    @staticmethod
    def extendMatrixRepresentation(operator, vectors, opMat):
        ket = vectors[-1].applyOp(operator)
        col = HipVector._multi_dot(vectors, ket)
        m = len(vectors)
        M = np.empty((m, m), dtype=np.float64)
        M[:m - 1, :m - 1] = opMat
        M[:, m - 1] = col
        M[m - 1, :] = col
        return M


class HipComplexVector(AbstractVector):
    """complex128 vector on the device: two real fp64 halves (``re``, ``im``), every operation built from
    the real kernels on the halves (the operator is real, so ``H (a + i b) = H a + i H b``).

    It is what ``HipVector(array)`` returns for a complex array - the counterpart of a ``NumpyVector`` with a
    complex dtype (numpyVector.py:25-28, 89-93: ``vdot`` conjugates ``self`` unless ``conjugate=False``) -,
    what ``HipVector.solve`` returns for a complex shift (feast.py:90) and what a complex scalar times a
    ``HipVector`` gives (feast.py:91-92).  Same constructor convention as the other backends:
    ``HipComplexVector(complex_ndarray, options)``; internally also ``HipComplexVector(re_vec, im_vec)``."""

    def __init__(self, re, im=None, ctx=None):
        if isinstance(re, HipVector):
            self.re, self.im = re, im
        else:
            host = np.asarray(re, dtype=np.complex128)
            opts = im if isinstance(im, dict) or im is None else None
            self.re = HipVector(np.ascontiguousarray(host.real), opts, ctx=ctx)
            self.im = HipVector(np.ascontiguousarray(host.imag), self.re.options, ctx=ctx)
        self.options = self.re.options
        self.ctx = self.re.ctx
        self.size = self.re.size
        self.shape = self.re.shape
        self.last_solve_stats = None

    @staticmethod
    def fromArray(template, array):
        return HipComplexVector(np.asarray(array, dtype=np.complex128), template.options, ctx=template.ctx)

    @staticmethod
    def _parts(v):
        """(re, im) halves of a complex or real device vector (im is None for a real one)."""
        return (v.re, v.im) if isinstance(v, HipComplexVector) else (v, None)

    # ---- properties ----------------------------------------------------------------
    @property
    def hasExactAddition(self):
        return True

    @property
    def dtype(self):
        return np.dtype(np.complex128)

    @property
    def maxD(self):
        return 0

    @property
    def array(self):
        return self.re.array + 1j * self.im.array

    def __len__(self):
        return len(self.re)

    # ---- arithmetic ------------------------------------------------------------------
    def _scaled(self, alpha):
        a = complex(alpha)
        re = HipVector.linearCombination([self.re, self.im], [a.real, -a.imag])
        im = HipVector.linearCombination([self.re, self.im], [a.imag, a.real])
        return HipComplexVector(re, im)

    def __mul__(self, other):
        return self._scaled(other)

    def __rmul__(self, other):
        return self._scaled(other)

    def __truediv__(self, other):
        return self._scaled(1.0 / complex(other))

    def __imul__(self, other):
        raise NotImplementedError          # numpyVector.py:66-67

    def __itruediv__(self, other):
        raise NotImplementedError          # numpyVector.py:69-70

    # ---- instance methods ------------------------------------------------------------
    def norm(self):
        return float(np.hypot(self.re.norm(), self.im.norm()))

    def normalize(self):
        nrm = self.norm()
        for half in (self.re, self.im):    # in place: aliases of this vector see the change (numpyVector.py:76-78)
            _lib.call("hipeig_divide", self.ctx.handle, half._buf.n, nrm, half._buf.ptr, half._buf.ptr)
        return self

    def real(self):
        return self.re.copy()

    def conjugate(self):
        return HipComplexVector(self.re.copy(), self.im * -1.0)

    def vdot(self, other, conjugate=True):
        """numpyVector.py:89-93: ``np.vdot`` (self conjugated) or the bilinear ``np.dot``."""
        br, bi = self._parts(other)
        rr, ir = self.re.vdot(br), self.im.vdot(br)
        ri, ii = (self.re.vdot(bi), self.im.vdot(bi)) if bi is not None else (0.0, 0.0)
        if conjugate:
            return complex(rr + ii, ri - ir)
        return complex(rr - ii, ri + ir)

    def copy(self):
        return HipComplexVector(self.re.copy(), self.im.copy())

    def applyOp(self, other):
        if not isinstance(other, HipCsrOperator):
            raise TypeError("HipComplexVector.applyOp needs a HipCsrOperator (device-resident CSR)")
        out_r, out_i = self.re.ctx.alloc(other.nrows), self.re.ctx.alloc(other.nrows)
        other.apply_pair(self.re._buf, self.im._buf, out_r, out_i)
        return HipComplexVector(self.re._new(out_r), self.im._new(out_i))

    def compress(self):
        return self

    # ---- static hooks ------------------------------------------------------------------
    @staticmethod
    def linearCombination(vectors, coeffs):
        assert len(vectors) == len(coeffs)
        vs_re, cs_re, vs_im, cs_im = [], [], [], []
        for v, c in zip(vectors, coeffs):
            c = complex(c)
            vr, vi = HipComplexVector._parts(v)
            vs_re.append(vr); cs_re.append(c.real)          # Re: cr vr - ci vi
            vs_im.append(vr); cs_im.append(c.imag)          # Im: ci vr + cr vi
            if vi is not None:
                vs_re.append(vi); cs_re.append(-c.imag)
                vs_im.append(vi); cs_im.append(c.real)
        return HipComplexVector(HipVector.linearCombination(vs_re, cs_re), HipVector.linearCombination(vs_im, cs_im))

    @staticmethod
    def orthogonalize_against_set(x, qs, lindep=LINDEP_DEFAULT_VALUE):
        """The reference's sweep, numpyVector.py:121-145, with its bilinear products."""
        for q in qs:
            t1 = x.vdot(q, conjugate=False)
            t2 = q.vdot(q, conjugate=False)
            x = HipComplexVector.linearCombination([x, q * (t1 / t2)], [1.0, -1.0])
        ip = np.complex128(x.vdot(x, conjugate=False))
        if ip > lindep:                                       # NumPy orders complex numbers lexicographically, as in the reference
            return x / np.sqrt(ip)
        return None

    @staticmethod
    def solve(H, b, sigma, x0=None, opType="her", reverseGF=False):
        """(sigma I - H) x = b for a complex right-hand side.  Real shift with MINRES: the real operator acts on
        the halves separately, so the two real systems go through ``solveBlock`` - which solves TWO right-hand sides one
        after the other (the lock-step block kernel pays from three on, ``BLOCK_SOLVE_MIN``); everything else is complex
        GCROT on (re, im) pairs, like a complex shift."""
        if not isinstance(H, HipCsrOperator):
            raise TypeError("HipComplexVector.solve needs a HipCsrOperator (device-resident CSR)")
        o = b.options["linearSystemArgs"]
        _preconditioner(o, sigma, x0, b.ctx)
        _gcrot_preconditioner(o, x0, b.ctx, H)
        if o["linearSolver"] == "minres_shifted":
            raise NotImplementedError("linearSolver='minres_shifted' takes a real right-hand side (its Lanczos run is real)")
        if o["linearSolver"] == "pardiso":
            return HipVector._solve_exact_small(H, b, sigma, reverseGF)
        is_complex_shift = isinstance(sigma, complex) or np.iscomplexobj(sigma)
        if x0 is not None and not isinstance(x0, (HipVector, HipComplexVector)):
            x0 = HipVector(np.asarray(x0), ctx=b.ctx)
        if o["linearSolver"] == "minres" and not is_complex_shift:
            if x0 is None:
                xr, xi = HipVector.solveBlock(H, [b.re, b.im], sigma, reverseGF=reverseGF)
            else:                                       # the real operator acts on the halves separately: so does the guess
                g_re, g_im = (x0.re, x0.im) if isinstance(x0, HipComplexVector) else (x0, x0 * 0.0)
                xr = HipVector.solve(H, b.re, sigma, g_re, reverseGF=reverseGF)
                xi = HipVector.solve(H, b.im, sigma, g_im, reverseGF=reverseGF)
            res = HipComplexVector(xr, xi)
            res.last_solve_stats = b.last_solve_stats = {"re": xr.last_solve_stats, "im": xi.last_solve_stats,
                                                         "iterations": max(xr.last_solve_stats["iterations"],
                                                                           xi.last_solve_stats["iterations"])}
            return res
        return HipVector._solve_complex(H, b, complex(sigma), o, reverseGF, x0)

    @staticmethod
    def _gram(A, B):
        """A^H B for lists of (possibly complex) vectors: four real Gram blocks on the matrix cores."""
        ar = [HipComplexVector._parts(v)[0] for v in A]
        ai = [HipComplexVector._parts(v)[1] for v in A]
        br = [HipComplexVector._parts(v)[0] for v in B]
        bi = [HipComplexVector._parts(v)[1] for v in B]

        def g(X, Y):
            if any(v is None for v in X) or any(v is None for v in Y):
                return np.zeros((len(X), len(Y)))
            out = np.empty((len(X), len(Y)))
            tx, k1 = _ptr_table([v._buf for v in X])
            ty, k2 = _ptr_table([v._buf for v in Y])
            _lib.call("hipeig_gram", X[0].ctx.handle, X[0]._buf.n, len(X), tx, len(Y), ty, out.ctypes.data_as(C.POINTER(C.c_double)))
            return out
        return (g(ar, br) + g(ai, bi)) + 1j * (g(ar, bi) - g(ai, br))

    @staticmethod
    def overlapMatrix(vectors):
        S = HipComplexVector._gram(vectors, vectors)
        return np.triu(S) + np.triu(S, 1).conj().T           # upper triangle mirrored, numpyVector.py:199-202

    @staticmethod
    def matrixRepresentation(operator, vectors):
        kets = [v.applyOp(operator) for v in vectors]
        M = HipComplexVector._gram(vectors, kets)
        return np.tril(M) + np.tril(M, -1).conj().T           # lower triangle mirrored, numpyVector.py:186-189

    @staticmethod
    def extendOverlapMatrix(vectors, overlap):
        col = HipComplexVector._gram(vectors, vectors[-1:])[:, 0]
        m = len(vectors)
        S = np.empty((m, m), dtype=np.complex128)
        S[:m - 1, :m - 1] = overlap
        S[:, m - 1] = col
        S[m - 1, :m - 1] = col[:-1].conj()
        return S

    @staticmethod
    def extendMatrixRepresentation(operator, vectors, opMat):
        col = HipComplexVector._gram(vectors, [vectors[-1].applyOp(operator)])[:, 0]
        m = len(vectors)
        M = np.empty((m, m), dtype=np.complex128)
        M[:m - 1, :m - 1] = opMat
        M[:, m - 1] = col
        M[m - 1, :m - 1] = col[:-1].conj()
        return M
