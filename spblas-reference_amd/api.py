"""Host-side mirror of the spblas-reference operator interface for the multiply() path.

Same names, argument meaning and error behaviour as the reference (paths relative to
/root/reference/include/spblas/):

  csr_view / csc_view          views/csr_view.hpp:12-77, views/csc_view.hpp
  scaled / scaled_view         algorithms/scaled.hpp, views/scaled_view_impl.hpp:97-219
  conjugated                   views/conjugated_view_impl.hpp: taken for complex SpMV / SpMM operands (conj(A),
                               conj(x / B) or both, in the kernels); a conjugated REAL operand is rejected with
                               RuntimeError like the GPU slot does (vendor/rocsparse/detail/spmv_impl.hpp:29-33)
  transposed                   algorithms/transposed.hpp:7-21 (zero-copy CSR<->CSC relabel)
  matrix_opt                   views/matrix_opt_impl.hpp:14-93 (caches the inspect result)
  operation_info_t             detail/operation_info_t.hpp:28-104
  spgemm_state_t               vendor/rocsparse/multiply_spgemm.hpp:28-230
  multiply, multiply_inspect   algorithms/multiply.hpp, vendor/rocsparse/detail/spmv_impl.hpp:18-90,
                               vendor/onemkl_sycl/spmm_impl.hpp:40-198
  multiply_compute/_fill, multiply_symbolic_compute/_fill, multiply_numeric
                               algorithms/multiply.hpp:48-55, vendor/rocsparse/multiply_spgemm.hpp:232-317

The reference is C++; its toolchain dependencies (range-v3, mdspan) are absent from
this image, so the C++ header layer (include/spblas/vendor/gfx950/) cannot be
exercised here and this Python layer is what the tests drive.  Device memory is
held in torch CUDA tensors (plumbing only): a view wraps caller-owned tensors exactly
as csr_view wraps caller-owned device pointers.  All compute goes through the C ABI
(include/spblas_gfx950.h); nothing here computes on the CPU or through torch ops.

Value types: float32 / float64 everywhere; complex64 / complex128 (std::complex<float / double>) for SpMV and SpMM on a
csr_view with int32 column indices (int32 / int64 row offsets), plan-free or inspected (VECTOR / ROWBLOCK / AUTO plans,
matrix_opt).  Complex operands may be conjugated -- conjugated(A), conjugated(x / B), or a tensor whose lazy conj bit is set
(t.conj(): the bit is folded into the kernel's flag, nothing is copied) -- and scaled by complex factors: a factor counts
conjugated iff an odd number of conjugated views wrap it (conjugated(scaled(s, A)) = conj(s) conj(A)).  Everything else with
complex values -- csc_view / transposed() operands, int64 column indices, SpGEMM, add, transpose, scale, triangular_solve,
triangular_solve_sweeps, ilu0, ilu0_sweeps, multicolor_order, permute, permute_vector, gauss_seidel -- raises TypeError; an output
with the conj bit set raises ValueError.

16-bit values: float16 / bfloat16 for SpMV and SpMM on a csr_view with int32 column indices (int32 / int64 row offsets),
plan-free or inspected (VECTOR / ROWBLOCK / AUTO plans, matrix_opt), scaled() by real factors.  A, x / B and y / C share the
one 16-bit type; products and sums are formed in fp32 and every output element is rounded once.  Everything else with 16-bit
values -- csc_view / transposed() operands, int64 column indices, mixed value types, a complex scaled() factor, conjugated
views, SpGEMM, add, transpose, scale, triangular_solve, triangular_solve_sweeps, ilu0, ilu0_sweeps, multicolor_order,
permute, permute_vector, gauss_seidel, the multi-GPU classes -- raises
TypeError (conjugated views: RuntimeError, as for real operands).
"""
import ctypes
import threading
import weakref

import numpy as np
import torch

from . import _capi
from ._capi import check


# --------------------------------------------------------------------------- views
class index(tuple):
    """spblas::index<I> (detail/index.hpp:14-55): a (rows, cols) pair."""

    def __new__(cls, a, b=None):
        if b is None:
            a, b = a
        return super().__new__(cls, (int(a), int(b)))


def _is_tensor(t):
    return isinstance(t, torch.Tensor)


class view_base:
    pass


class csr_view(view_base):
    """Non-owning CSR view over caller-owned device arrays (views/csr_view.hpp:20-26)."""

    def __init__(self, values, rowptr, colind, shape, nnz):
        self._values, self._rowptr, self._colind = values, rowptr, colind
        self._shape, self._nnz = index(shape), int(nnz)

    def update(self, values, rowptr, colind, shape=None, nnz=None):  # csr_view.hpp:36-49
        self._values, self._rowptr, self._colind = values, rowptr, colind
        if shape is not None:
            self._shape, self._nnz = index(shape), int(nnz)

    def values(self):
        return self._values

    def rowptr(self):
        return self._rowptr

    def colind(self):
        return self._colind

    def shape(self):
        return self._shape

    def size(self):
        return self._nnz


class csc_view(view_base):
    """Non-owning CSC view (views/csc_view.hpp)."""

    def __init__(self, values, colptr, rowind, shape, nnz):
        self._values, self._colptr, self._rowind = values, colptr, rowind
        self._shape, self._nnz = index(shape), int(nnz)

    def update(self, values, colptr, rowind, shape=None, nnz=None):  # views/csc_view.hpp
        self._values, self._colptr, self._rowind = values, colptr, rowind
        if shape is not None:
            self._shape, self._nnz = index(shape), int(nnz)

    def values(self):
        return self._values

    def colptr(self):
        return self._colptr

    def rowind(self):
        return self._rowind

    def shape(self):
        return self._shape

    def size(self):
        return self._nnz


class scaled_view(view_base):
    def __init__(self, alpha, base):
        self._alpha, self._base = alpha, base

    def alpha(self):
        return self._alpha

    def base(self):
        return self._base

    def shape(self):
        return _shape_of(self._base)


class conjugated_view(view_base):
    def __init__(self, base):
        self._base = base

    def base(self):
        return self._base

    def shape(self):
        return _shape_of(self._base)


class matrix_opt(view_base):
    """matrix_opt<M> (views/matrix_opt_impl.hpp): owns the cached vendor handle -- here
    the SpMV/SpMM plan built by multiply_inspect."""

    def __init__(self, matrix):
        if not isinstance(matrix, (csr_view, csc_view)):
            raise TypeError("matrix_opt wraps a csr_view or csc_view")
        self.matrix_ = matrix
        self._plan = None

    def base(self):
        return self.matrix_

    def shape(self):
        return self.matrix_.shape()

    def size(self):
        return self.matrix_.size()


def scaled(alpha, t):
    return scaled_view(alpha, t)


def conjugated(t):
    return conjugated_view(t)


def transposed(a):
    """algorithms/transposed.hpp:7-21: re-label CSR<->CSC with zero copy."""
    if isinstance(a, csr_view):
        return csc_view(a.values(), a.rowptr(), a.colind(), (a.shape()[1], a.shape()[0]), a.size())
    if isinstance(a, csc_view):
        return csr_view(a.values(), a.colptr(), a.rowind(), (a.shape()[1], a.shape()[0]), a.size())
    raise TypeError("transposed() expects a csr_view or csc_view")


# ----------------------------------------------------------- detail/view_inspectors.hpp
def get_ultimate_base(t):  # view_inspectors.hpp:104-111
    while isinstance(t, (scaled_view, conjugated_view, matrix_opt)):
        t = t.base()
    return t


def get_scaling_factor(*ts):  # view_inspectors.hpp:22-77: product of all factors, or None
    out = None
    for t in ts:
        while isinstance(t, (scaled_view, conjugated_view, matrix_opt)):
            if isinstance(t, scaled_view):
                out = t.alpha() if out is None else out * t.alpha()
            t = t.base()
    return out


def is_conjugated(t):  # view_inspectors.hpp:81-97: odd number of conjugated_views
    c = False
    while isinstance(t, (scaled_view, conjugated_view, matrix_opt)):
        if isinstance(t, conjugated_view):
            c = not c
        t = t.base()
    return c


def has_matrix_opt(t):  # view_inspectors.hpp:113-122
    while isinstance(t, (scaled_view, conjugated_view, matrix_opt)):
        if isinstance(t, matrix_opt):
            return True
        t = t.base()
    return False


def _get_matrix_opt(t):
    while isinstance(t, (scaled_view, conjugated_view, matrix_opt)):
        if isinstance(t, matrix_opt):
            return t
        t = t.base()
    return None


def _shape_of(t):
    if _is_tensor(t):
        return t.shape[0] if t.dim() == 1 else index(t.shape[0], t.shape[1])
    return t.shape()


# --------------------------------------------------------------------------- state
class _Handle:
    """One backend handle per (host thread, device).  A handle carries the stream the next call launches on and a
    scratch buffer, so -- like the vendor handles it stands in for (vendor/rocsparse/detail/operation_state_t.hpp keeps
    one per operation state) -- it must not be shared by threads that call concurrently: ctypes drops the GIL for the
    duration of a call, and a second thread re-binding the stream between this thread's set_stream and its launch
    would put the launch on the wrong stream."""
    _tls = threading.local()

    def __init__(self, device):
        self.device = device
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            check(_capi.lib().spblas_gfx950_create(ctypes.byref(h), None), "spblas_gfx950_create")
        self.h = h

    def __del__(self):  # a thread's handles go with the thread (plans and states keep theirs alive)
        try:
            if self.h:
                _capi.lib().spblas_gfx950_destroy(self.h)
                self.h = None
        except Exception:
            pass  # interpreter shutdown

    def set_option(self, option, value):
        check(_capi.lib().spblas_gfx950_set_option(self.h, option, value), "spblas_gfx950_set_option")

    def spmv_t_last(self, with_items=True):
        """What the last un-inspected transposed multiply on this handle did (spblas_gfx950_spmv_t_last; a diagnostic, like
        _Plan.info): path 'none' / 'scatter' / 'two_pass', why the scatter kernel ran, the slice width W, the slices S, the
        tiles and the segment length the decision was made on.  with_items also copies the number of work items of the
        accumulate pass back, which SYNCHRONISES the stream of that call (-1 where there is none to report)."""
        arr = (ctypes.c_int64 * 8)()
        check(_capi.lib().spblas_gfx950_spmv_t_last(self.h, arr, 8 if with_items else 7), "spblas_gfx950_spmv_t_last")
        out = {"path": ("none", "scatter", "two_pass")[arr[0]],
               "why": (None, "not_wanted", "does_not_fit", "capturing", "no_scratch")[arr[1]],
               "W": arr[2], "S": arr[3], "ntile": arr[4], "seg": arr[5], "w_hook_ignored": arr[6]}
        if with_items:
            out["n_items"] = arr[7]
        return out

    def sptrsm_last(self):
        """What the last triangular solve with a block of right-hand sides on this handle decided (spblas_gfx950_sptrsm_last;
        a diagnostic, host integers only): path 0 none yet, 1 forwarded to the vector solve, 2 element kernels, 3 16-byte
        pieces; X's misalignment in elements, the units per row, log2 of the unit lanes C and the entry lanes E of a team,
        whether B is read in pieces, the bytes X's buffer descriptor spans and the passes ceil(units / C) of the unit loop."""
        arr = (ctypes.c_int64 * 8)()
        check(_capi.lib().spblas_gfx950_sptrsm_last(self.h, arr, 8), "spblas_gfx950_sptrsm_last")
        return dict(zip(("path", "mis", "units", "logC", "E", "b_piece", "x_bytes", "passes"), list(arr)))

    @classmethod
    def current(cls, device):
        if device.type != "cuda":
            raise RuntimeError("gfx950 backend: arrays must live in device (HIP) memory; there is no CPU fallback")
        key = device.index if device.index is not None else torch.cuda.current_device()
        by_device = getattr(cls._tls, "by_device", None)
        if by_device is None:
            by_device = cls._tls.by_device = {}
        hd = by_device.get(key)
        if hd is None:
            hd = by_device[key] = cls(key)
        stream = torch.cuda.current_stream(key).cuda_stream
        check(_capi.lib().spblas_gfx950_set_stream(hd.h, ctypes.c_void_p(stream)), "spblas_gfx950_set_stream")
        return hd


# In-place changes to an array made through this module's own raw kernels (invisible to torch's version
# counter) are recorded here: data_ptr -> number of such writes.  Every API entry that writes a value or column
# array through the C ABI -- scale(), multiply_fill / multiply_numeric, add, transpose -- bumps the epoch, so a
# SLICED plan's value snapshot and the "colind provably untouched" test of repeated SpGEMM fills see them.
_value_epochs = {}


def _note_write(*tensors):
    for t in tensors:
        if t is not None:
            _value_epochs[t.data_ptr()] = _value_epochs.get(t.data_ptr(), 0) + 1


def _values_stamp(values):
    """(data_ptr, torch version counter, scale() epoch): changes whenever the array is rebound or modified in
    place through torch or through this module."""
    return values.data_ptr(), values._version, _value_epochs.get(values.data_ptr(), 0)


class _Plan:
    """Owner of a spblas_gfx950_plan_t (released with the handle's stream order).

    Holds references to the matrix's tensors, so their addresses -- the plan's identity in the library -- cannot
    be recycled for another matrix while the plan lives.  A SLICED plan multiplies with a re-tiled COPY of the
    values (include/spblas_gfx950.h, "value snapshot contract"); `stamp` remembers the state of the caller's
    value array the copy was taken from, and _spmv refreshes the copy when it sees another one."""

    def __init__(self, handle, plan, key, tensors=None):
        self.handle, self.plan, self.key = handle, plan, key
        self.tensors = tensors
        self.snapshot = self.info()["alg"] == _capi.SPMV_SLICED
        self.stamp = _values_stamp(tensors[2]) if tensors is not None and tensors[2] is not None else None

    def _calling_handle(self, device=None):
        """The CALLING thread's handle, bound to its current stream: a plan made in thread A and used in thread B (an
        autograd backward thread, a worker pool) must launch its refresh / inspect work on B's stream, in order with B's
        multiply -- not on whatever stream A's handle was last bound to.  The creator's handle (self.handle) is kept
        alive for the plan's destruction only."""
        return _Handle.current(device if device is not None else torch.device("cuda", self.handle.device))

    def refresh_if_stale(self, values):
        """SLICED plans only: re-copy the values when the caller's array was rebound or changed in place through
        torch or scale() since the copy was taken.  (Writes by foreign kernels are invisible here: call
        update_values after those, as the C ABI asks.)"""
        if self.snapshot and values is not None and _values_stamp(values) != self.stamp:
            self.update_values(values)

    def info(self):
        arr = (ctypes.c_int64 * 12)()
        check(_capi.lib().spblas_gfx950_plan_info(self.plan, arr), "spblas_gfx950_plan_info")
        names = ["alg", "window", "n_windows", "n_long_rows", "max_row_len", "device_bytes", "n_slices",
                 "empty_rows", "rows_per_bin", "bin_aligned", "expand_items", "reduce_items"]
        return dict(zip(names, list(arr)))

    def sliced_info(self):
        arr = (ctypes.c_int64 * 12)()
        check(_capi.lib().spblas_gfx950_plan_info_sliced(self.plan, arr), "spblas_gfx950_plan_info_sliced")
        names = ["n_bins", "variable_bins", "expand_blocks", "reduce_blocks", "placed_entries", "hub_rows", "hub_len",
                 "ksplit", "tiled_rows", "auto_trial", "trial_rowblock_ns", "trial_sliced_ns"]
        d = dict(zip(names, list(arr)))
        bits = d["auto_trial"]
        d["row_code_u8"] = (bits >> 1) & 1  # one-byte row codes in the reduce's stream (runs sorted by row)
        d["refresh_each_call"] = (bits >> 6) & 1  # made without the snapshot opt-in: every multiply takes A's values again
        d["value_free"] = (bits >> 7) & 1  # ... and holds no copy of them: the reduce reads the caller's array through LDS (round 5)
        d["nt_product_stores"] = (bits >> 2) & 1  # the expand stores its products with the non-temporal hint
        d["store_trial"] = (bits >> 3) & 1  # THIS plan timed both store flavours (opt-in: OPT_STORE_TRIAL = 2 on the handle or SPBLAS_GFX950_PB_NT=-2)
        d["auto_trial"] = bits & 1
        if (bits >> 4) & 1:  # hot-column split (csrc/spmv_hot.hip): the tile numbers above are those of A_rest
            hot = (ctypes.c_int64 * 8)()
            check(_capi.lib().spblas_gfx950_plan_info_hot(self.plan, hot), "spblas_gfx950_plan_info_hot")
            d["hot_split"] = dict(zip(("hot_columns", "hot_entries", "hot_rows", "hot_long_rows", "tiled_entries",
                                       "tiled_device_bytes", "windows"), list(hot)))
        if d["store_trial"] and not d["auto_trial"]:  # (the two time slots carry AUTO's trial when both ran)
            d["store_trial_ns"] = {"plain": d.pop("trial_rowblock_ns"), "non_temporal": d.pop("trial_sliced_ns")}
            d["trial_rowblock_ns"] = d["trial_sliced_ns"] = 0
        return d

    # two-stage execution of a SLICED plan (include/spblas_gfx950.h: spmv_expand / spmv_reduce_rows)
    def bind_stages(self, x, y_base_ptr, dtype, alpha=1.0, beta=0.0):
        """Returns (expand, reduce_rows) callables with every argument pre-bound; reduce_rows(lo, hi)
        finishes the row-bins starting in [lo, hi).  y_base_ptr is the address of local row 0."""
        lib = _capi.lib()
        ct = _VT[dtype][1]
        a, b = ct(alpha), ct(beta)
        # (the BINDING thread's handle: the callables belong to the thread that bound them)
        hd = _Handle.current(x.device)
        h, p, xp, yp = hd.h, self.plan, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y_base_ptr)
        keep = (a, b, x, hd)
        # the stream that is current NOW: every other API call re-binds the handle to the then-current stream, so
        # the bound callables put the handle back on theirs before they launch
        stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        set_stream = lib.spblas_gfx950_set_stream

        def expand():
            set_stream(h, stream)
            check(lib.spblas_gfx950_spmv_expand(h, p, xp), "spmv_expand")

        def reduce_rows(lo, hi, _keep=keep):
            set_stream(h, stream)
            check(lib.spblas_gfx950_spmv_reduce_rows(h, p, ctypes.byref(a), ctypes.byref(b), yp, lo, hi),
                  "spmv_reduce_rows")

        return expand, reduce_rows

    def spmm_inspect(self):
        """The SpMM part of multiply_inspect (spblas_gfx950_spmm_inspect): column-locality probe of every block of
        32 rows; qualifying blocks go to the LDS-staged matrix-core kernel, long rows are cut into parts."""
        check(_capi.lib().spblas_gfx950_spmm_inspect(self._calling_handle().h, self.plan), "multiply_inspect")
        return self

    def spmm_info(self):
        arr = (ctypes.c_int64 * 4)()
        check(_capi.lib().spblas_gfx950_spmm_plan_info(self.plan, arr), "spblas_gfx950_spmm_plan_info")
        return dict(zip(("inspected", "panel_blocks", "panel_nnz", "long_rows"), list(arr)))

    def spmm_blocks(self):
        """What the SpMM inspect decided, block by block (spblas_gfx950_spmm_plan_blocks; a diagnostic, like spmm_info):
        the counts, and per block of 32 rows its kind (0 row-group kernel, 1 entry loop / tile kernel, 2 matrix cores), its
        column window (nblk x 2) and its tile table (nblk x 17: count, then ascending tile ids) as numpy arrays.
        SYNCHRONISES the calling thread's stream.  All counts zero and empty arrays for a plan the probe did not run on."""
        names = ("inspected", "nblk", "npanel", "ndense", "panel_nnz", "band", "band_ch", "band_waves", "band_dense_pm",
                 "min_per_tile")
        fn, h = _capi.lib().spblas_gfx950_spmm_plan_blocks, self._calling_handle().h
        arr = (ctypes.c_int64 * 10)()
        check(fn(h, self.plan, arr, None, None, None), "spblas_gfx950_spmm_plan_blocks")
        nblk = int(arr[1])
        kind, win, tiles = np.zeros(nblk, np.uint8), np.zeros((nblk, 2), np.int32), np.zeros((nblk, 17), np.int32)
        if nblk:
            check(fn(h, self.plan, arr, kind.ctypes.data, win.ctypes.data, tiles.ctypes.data), "spblas_gfx950_spmm_plan_blocks")
        out = dict(zip(names, list(arr)))
        out.update(kind=kind, win=win, tiles=tiles)
        return out

    def hot_layout(self):
        """What the inspect laid out for the hot-column part of a split SLICED plan (spblas_gfx950_plan_hot_layout; a
        diagnostic, like spmm_blocks): the counts, and as numpy arrays the hot columns (ascending), the rows of y that have
        hot entries, their offsets into A_hot (int64), the first row of every window and the rows that lie in more than one
        window (sorted here: the device lists them in the order of an atomic).  SYNCHRONISES the calling thread's stream.
        All counts zero and empty arrays for a plan without the split."""
        names = ("thr", "k", "n_hot", "m_hot", "nwin", "n_cross", "grid", "depth")
        fn, h = _capi.lib().spblas_gfx950_plan_hot_layout, self._calling_handle().h
        arr = (ctypes.c_int64 * 8)()
        check(fn(h, self.plan, arr, None, None, None, None, None), "spblas_gfx950_plan_hot_layout")
        out = dict(zip(names, list(arr)))
        split = out["k"] > 0
        cols, rows = np.zeros(out["k"], np.int32), np.zeros(out["m_hot"], np.int32)
        rowptr = np.zeros(out["m_hot"] + 1 if split else 0, np.int64)
        win_row = np.zeros(out["nwin"] + 1 if split else 0, np.int32)
        cross = np.zeros(out["n_cross"], np.int32)
        if split:
            check(fn(h, self.plan, arr, cols.ctypes.data, rows.ctypes.data, rowptr.ctypes.data, win_row.ctypes.data,
                     cross.ctypes.data), "spblas_gfx950_plan_hot_layout")
        out.update(hot_cols=cols, hot_rows=rows, hot_rowptr=rowptr, win_row=win_row, cross_rows=np.sort(cross))
        return out

    def update_values(self, values):
        """Refresh the plan after A's values changed in place (only the SLICED re-tiling keeps
        a copy of them; the other algorithms read the caller's array on every call)."""
        check(_capi.lib().spblas_gfx950_spmv_plan_update_values(self._calling_handle(values.device).h, self.plan,
                                                                _ptr(values)), "update_values")
        self.stamp = _values_stamp(values)
        if self.tensors is not None:
            self.tensors = (self.tensors[0], self.tensors[1], values)

    def __del__(self):
        try:
            if self.plan:
                _capi.lib().spblas_gfx950_plan_destroy(self.handle.h, self.plan)
                self.plan = None
        except Exception:
            pass


class operation_info_t:
    """detail/operation_info_t.hpp:28-104: result_shape(), result_nnz(), backend state_."""

    def __init__(self, result_shape=(0, 0), result_nnz=0, state=None):
        self._result_shape, self._result_nnz = index(result_shape), int(result_nnz)
        self.state_ = state

    def result_shape(self):
        return self._result_shape

    def result_nnz(self):
        return self._result_nnz

    def update_impl_(self, result_shape, result_nnz):
        self._result_shape, self._result_nnz = index(result_shape), int(result_nnz)


class spgemm_state_t:
    """vendor/rocsparse/multiply_spgemm.hpp:28-230."""

    def __init__(self):
        self._handle = None
        self._state = None
        self._result_shape = index(0, 0)
        self._result_nnz = 0

    def result_shape(self):
        return self._result_shape

    def result_nnz(self):
        return self._result_nnz

    def _ensure(self, device):
        hd = _Handle.current(device)  # the CALLING thread's handle on its current stream (the state itself is handle-free)
        if self._state is None:
            self._handle = hd  # kept alive for the state's destruction
            st = ctypes.c_void_p()
            check(_capi.lib().spblas_gfx950_spgemm_create(hd.h, ctypes.byref(st)), "spblas_gfx950_spgemm_create")
            self._state = st
        return hd, self._state

    def info(self):
        """Introspection (spblas_gfx950_spgemm_info): which kernels the numeric passes of this state take."""
        if self._state is None:
            return {}
        raw = (ctypes.c_int64 * 8)()
        check(_capi.lib().spblas_gfx950_spgemm_info(self._state, raw), "spblas_gfx950_spgemm_info")
        return {"nnz_c": raw[0], "wave_per_row_rows": raw[1], "direct_rows": raw[2], "fills_by_rank": bool(raw[3]),
                "lanes_per_b_row": raw[4], "bin1_rows": raw[5], "bin3_rows": raw[6], "dense_rows": raw[7]}

    def __del__(self):
        try:
            if self._state:
                _capi.lib().spblas_gfx950_spgemm_destroy(self._handle.h, self._state)
                self._state = None
        except Exception:
            pass


# --------------------------------------------------------------------------- helpers
class _c_complex(ctypes.Structure):
    """One complex host scalar (alpha / beta of a complex call): interleaved (re, im) like std::complex."""

    def __init__(self, v=0):
        v = complex(v)
        super().__init__(v.real, v.imag)


class c_complex64(_c_complex):
    _fields_ = [("re", ctypes.c_float), ("im", ctypes.c_float)]


class c_complex128(_c_complex):
    _fields_ = [("re", ctypes.c_double), ("im", ctypes.c_double)]


_VT = {torch.float32: (_capi.F32, ctypes.c_float), torch.float64: (_capi.F64, ctypes.c_double),
       torch.complex64: (_capi.C32, c_complex64), torch.complex128: (_capi.C64, c_complex128),
       torch.float16: (_capi.F16, ctypes.c_float), torch.bfloat16: (_capi.BF16, ctypes.c_float)}
_COMPLEX = (torch.complex64, torch.complex128)
_LOWP = (torch.float16, torch.bfloat16)  # alpha / beta of a 16-bit call are float (fp32) scalars
_OT = {torch.int32: _capi.I32, torch.int64: _capi.I64}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(
        t.data_ptr() if t is not None else 0)


def _vtype(t, what, complex_ok=False, lowp_ok=False):
    if t.dtype in _COMPLEX and not complex_ok:
        raise TypeError(f"{what}: complex values are supported for SpMV / SpMM on csr_view operands only, got {t.dtype}")
    if t.dtype in _LOWP and not lowp_ok:
        raise TypeError(f"{what}: {t.dtype} values are supported for SpMV / SpMM on csr_view operands only")
    if t.dtype not in _VT:
        raise TypeError(f"{what}: gfx950 backend supports float32/float64 values (complex64/complex128, float16/bfloat16 "
                        f"for SpMV / SpMM), got {t.dtype}")
    return _VT[t.dtype]


def _lowp_dtype(t):
    """The 16-bit value type of an operand (a view's values or a dense tensor), else None."""
    base = get_ultimate_base(t)
    vals = base if _is_tensor(base) else (base.values() if hasattr(base, "values") else None)
    return vals.dtype if vals is not None and vals.dtype in _LOWP else None


def _reject_lowp(what, *ts):
    for t in ts:
        dt = _lowp_dtype(t) if t is not None else None
        if dt is not None:
            raise TypeError(f"{what}: {dt} values are supported for SpMV / SpMM on csr_view operands only")


def _lowp_operand(a, what):
    """The csr_view under a 16-bit operand; TypeError for everything out of scope."""
    a_base = get_ultimate_base(a)
    dt = _lowp_dtype(a) or "16-bit"
    if not isinstance(a_base, csr_view):
        raise TypeError(f"{what}: {dt} values take a csr_view operand (csc_view / transposed(): not supported)")
    if a_base.values() is None or a_base.values().dtype not in _LOWP:
        raise TypeError(f"{what}: A, x / B and y / C must share one 16-bit value type, got A of "
                        f"{None if a_base.values() is None else a_base.values().dtype}")
    if a_base.colind() is not None and a_base.colind().dtype != torch.int32:
        raise TypeError(f"{what}: {dt} values take int32 column indices only")
    _check_csr(a_base, what)
    return a_base


def _lowp_alpha(a, b):
    """alpha of a 16-bit call: the product of the scaled() factors, real only (a float scalar)."""
    f = get_scaling_factor(a, b)
    if f is None:
        return 1.0
    if isinstance(f, complex) or (_is_tensor(f) and f.is_complex()):
        raise TypeError(f"multiply: {_lowp_dtype(a) or _lowp_dtype(b)} operands take real scaled() factors only, got the "
                        f"complex factor {f}")
    return float(f)


def _spmv_lowp(info, a, b, c, prepare_only):
    """_spmv for float16 / bfloat16 operands (spblas_gfx950_spmv, lowp.hip)."""
    a_base, b_base = _lowp_operand(a, "multiply"), get_ultimate_base(b)
    _reject_conjugated(a, b, c)
    if not _is_tensor(c) or c.dim() != 1:
        raise TypeError("multiply: the output vector must be a plain 1-D device tensor")
    dt = a_base.values().dtype
    if b_base.dtype != dt or c.dtype != dt:
        raise TypeError(f"multiply: A, x and y must share one value type, got {dt}, {b_base.dtype}, {c.dtype}")
    if a_base.shape()[0] != c.shape[0] or a_base.shape()[1] != b_base.shape[0]:
        raise ValueError("multiply: matrix and vector dimensions are incompatible.")
    if not (b_base.is_contiguous() and c.is_contiguous()):
        raise ValueError("multiply: x and y must be contiguous")
    vt, ct = _vtype(a_base.values(), "multiply", lowp_ok=True)
    alpha, beta = ct(_lowp_alpha(a, b)), ct(0)
    hd = _Handle.current(c.device)
    plan = _find_plan(info, a, a_base)
    m, n = a_base.shape()
    args = (hd.h, plan.plan if plan else None, _capi.OP_N, m, n, a_base.size(), ctypes.byref(alpha), _ptr(a_base.rowptr()),
            _ptr(a_base.colind()), _ptr(a_base.values()), _ptr(b_base), ctypes.byref(beta), _ptr(c),
            _OT[a_base.rowptr().dtype], vt)
    if prepare_only:  # (the entry point with its bound arguments, and what keeps the operands alive)
        return (_capi.lib().spblas_gfx950_spmv, args), (alpha, beta, plan, a, b, c)
    check(_capi.lib().spblas_gfx950_spmv(*args), "multiply")


def _spmm_lowp(info, a, b, c):
    """_spmm for float16 / bfloat16 operands (spblas_gfx950_spmm_strided, lowp.hip)."""
    a_base, b_base = _lowp_operand(a, "multiply"), get_ultimate_base(b)
    _reject_conjugated(a, b, c)
    if not _is_tensor(c) or c.dim() != 2:
        raise TypeError("multiply: the output matrix must be a plain 2-D device tensor")
    dt = a_base.values().dtype
    if b_base.dtype != dt or c.dtype != dt:
        raise TypeError(f"multiply: A, B and C must share one value type, got {dt}, {b_base.dtype}, {c.dtype}")
    if (a_base.shape()[0] != c.shape[0] or b_base.shape[1] != c.shape[1]
            or a_base.shape()[1] != b_base.shape[0]):
        raise ValueError("multiply: matrix dimensions are incompatible.")
    vt, ct = _vtype(a_base.values(), "multiply", lowp_ok=True)
    m, k = a_base.shape()
    n = c.shape[1]
    (brs, bcs), (crs, ccs) = _dense_strides(b_base, k, n), _dense_strides(c, m, n)
    alpha, beta = ct(_lowp_alpha(a, b)), ct(0)
    plan = _find_plan(info, a, a_base)
    hd = _Handle.current(c.device)
    check(_capi.lib().spblas_gfx950_spmm_strided(hd.h, plan.plan if plan is not None else None, m, k, n, a_base.size(),
                                                 ctypes.byref(alpha), _ptr(a_base.rowptr()), _ptr(a_base.colind()),
                                                 _ptr(a_base.values()), _ptr(b_base), brs, bcs, ctypes.byref(beta), _ptr(c),
                                                 crs, ccs, _OT[a_base.rowptr().dtype], vt), "multiply")


def _is_complex_view(t):
    base = get_ultimate_base(t)
    vals = base if _is_tensor(base) else (base.values() if hasattr(base, "values") else None)
    return vals is not None and vals.dtype in _COMPLEX


def _reject_complex(what, *ts):
    if any(_is_complex_view(t) for t in ts if t is not None):
        raise TypeError(f"{what}: complex values are supported for SpMV / SpMM on csr_view operands only")


def complex_scaling_factor(*ts):
    """The scaling factor of complex operands: the product of every scaled() factor, each conjugated iff an odd number of
    conjugated views wrap it (views/conjugated_view_impl.hpp: a conjugated view yields conj of whatever its base yields, so
    conjugated(scaled(s, A)) is conj(s) * conj(A) while scaled(s, conjugated(A)) is s * conj(A)).  None without factors.
    (get_scaling_factor, view_inspectors.hpp:22-77, multiplies the factors as they are: right for real operands only.)"""
    out = None
    for t in ts:
        odd = False
        while isinstance(t, (scaled_view, conjugated_view, matrix_opt)):
            if isinstance(t, conjugated_view):
                odd = not odd
            elif isinstance(t, scaled_view):
                f = complex(t.alpha())
                f = f.conjugate() if odd else f
                out = f if out is None else out * f
            t = t.base()
    return out


def _complex_conj_flags(a, a_values, b, b_base, c):
    """conj_flags of spblas_gfx950_spmv_conj / spmm_strided_conj for complex operands: conjugated views (parity rule of
    is_conjugated) XOR the lazy conj bit of A's values and of x / B.  Returns (flags, x / B with its negative bit resolved)."""
    if c.is_conj() or c.is_neg():
        raise ValueError("multiply: the output must not be a lazily conjugated / negated tensor (resolve it first)")
    if is_conjugated(c):
        raise ValueError("multiply: the output cannot be a conjugated view")
    ca = is_conjugated(a) ^ bool(a_values.is_conj())
    cx = is_conjugated(b) ^ bool(b_base.is_conj())
    # (torch's negative bit is resolved -- a copy, made only when the bit is set; the conj bit is kept and folded in)
    return (_capi.CONJ_A if ca else 0) | (_capi.CONJ_X if cx else 0), a_values.resolve_neg(), b_base.resolve_neg()


def _complex_operand(a, what):
    a_base = get_ultimate_base(a)
    if not isinstance(a_base, csr_view):
        raise TypeError(f"{what}: complex values take a csr_view operand (csc_view / transposed(): not supported)")
    if a_base.colind() is not None and a_base.colind().dtype != torch.int32:
        raise TypeError(f"{what}: complex values take int32 column indices only")
    _check_csr(a_base, what)
    return a_base


def _spmv_complex(info, a, b, c, prepare_only):
    """_spmv for complex64 / complex128 operands (spblas_gfx950_spmv_conj)."""
    a_base, b_base = _complex_operand(a, "multiply"), get_ultimate_base(b)
    if not _is_tensor(c) or c.dim() != 1:
        raise TypeError("multiply: the output vector must be a plain 1-D device tensor")
    if a_base.shape()[0] != c.shape[0] or a_base.shape()[1] != b_base.shape[0]:
        raise ValueError("multiply: matrix and vector dimensions are incompatible.")
    vt, ct = _vtype(a_base.values(), "multiply", complex_ok=True)
    if b_base.dtype != a_base.values().dtype or c.dtype != a_base.values().dtype:
        raise TypeError("multiply: A, x and y must share one value type")
    if not (b_base.is_contiguous() and c.is_contiguous()):
        raise ValueError("multiply: x and y must be contiguous")
    flags, a_vals, x = _complex_conj_flags(a, a_base.values(), b, b_base, c)
    alpha_opt = complex_scaling_factor(a, b)
    alpha, beta = ct(1 if alpha_opt is None else alpha_opt), ct(0)
    hd = _Handle.current(c.device)
    plan = _find_plan(info, a, a_base)
    m, n = a_base.shape()
    args = (hd.h, plan.plan if plan else None, _capi.OP_N, m, n, a_base.size(), ctypes.byref(alpha), _ptr(a_base.rowptr()),
            _ptr(a_base.colind()), _ptr(a_vals), _ptr(x), ctypes.byref(beta), _ptr(c), _OT[a_base.rowptr().dtype], vt, flags)
    if prepare_only:  # (the entry point with its bound arguments, and what keeps the operands alive)
        return (_capi.lib().spblas_gfx950_spmv_conj, args), (alpha, beta, plan, a, b, c, a_vals, x)
    check(_capi.lib().spblas_gfx950_spmv_conj(*args), "multiply")


def _spmm_complex(info, a, b, c):
    """_spmm for complex64 / complex128 operands (spblas_gfx950_spmm_strided_conj)."""
    a_base, b_base = _complex_operand(a, "multiply"), get_ultimate_base(b)
    if not _is_tensor(c) or c.dim() != 2:
        raise TypeError("multiply: the output matrix must be a plain 2-D device tensor")
    if (a_base.shape()[0] != c.shape[0] or b_base.shape[1] != c.shape[1]
            or a_base.shape()[1] != b_base.shape[0]):
        raise ValueError("multiply: matrix dimensions are incompatible.")
    vt, ct = _vtype(a_base.values(), "multiply", complex_ok=True)
    if b_base.dtype != a_base.values().dtype or c.dtype != a_base.values().dtype:
        raise TypeError("multiply: A, B and C must share one value type")
    flags, a_vals, bb = _complex_conj_flags(a, a_base.values(), b, b_base, c)
    m, k = a_base.shape()
    n = c.shape[1]
    (brs, bcs), (crs, ccs) = _dense_strides(bb, k, n), _dense_strides(c, m, n)
    alpha_opt = complex_scaling_factor(a, b)
    alpha, beta = ct(1 if alpha_opt is None else alpha_opt), ct(0)
    plan = _find_plan(info, a, a_base)
    hd = _Handle.current(c.device)
    check(_capi.lib().spblas_gfx950_spmm_strided_conj(hd.h, plan.plan if plan is not None else None, m, k, n, a_base.size(),
                                                      ctypes.byref(alpha), _ptr(a_base.rowptr()), _ptr(a_base.colind()),
                                                      _ptr(a_vals), _ptr(bb), brs, bcs, ctypes.byref(beta), _ptr(c), crs, ccs,
                                                      _OT[a_base.rowptr().dtype], vt, flags), "multiply")


def _dense_strides(t, rows, n):
    """(row stride, column stride) of a layout_right or layout_left dense operand with `rows` rows and n columns."""
    if t.numel() == 0:
        return max(n, 1), 1
    rs, cs = t.stride(0), t.stride(1)
    if (cs == 1 or n <= 1) and (rows <= 1 or rs >= n):      # layout_right, possibly a column window (rs > n)
        return (rs if rows > 1 else max(n, 1)), 1
    if (rs == 1 or rows <= 1) and (n <= 1 or cs >= rows):   # layout_left, possibly a row window (cs > rows)
        return 1, (cs if n > 1 else max(rows, 1))
    raise ValueError("multiply: dense operands must be row-major (layout_right) or column-major (layout_left)")


# id of an int64 index tensor -> (weak reference to it, (its version, the range bound, the entry count) when narrowed, the copy)
_NARROWED = {}
_NARROWED_LOCK = threading.RLock()  # (re-entrant: a finaliser may run while this thread holds it)


def _index_version(idx):
    """torch's in-place edit counter of a tensor (copy_, idx[k] = v, any op with a trailing underscore bump it), or None for
    a tensor that keeps none (made under inference mode): such an array is narrowed afresh on every call."""
    try:
        return idx._version
    except RuntimeError:
        return None


def _int32_columns(a, what):
    """A csr_view / csc_view whose index array is int64 -- the slot this backend replaces admits them
    (vendor/rocsparse/types.hpp:16-24) -- as the same view over an int32 copy (spblas_gfx950_narrow_indices: ValueError if an
    index does not fit the other dimension).  The copy is made once per index tensor, version of its contents AND range
    bound (the same tensor in a view with a smaller other dimension is checked against that one), so that
    multiply_inspect and the multiplies that follow see ONE array (a plan is tied to its structure arrays) while a plan-free
    multiply reads the caller's indices as they are at the time of the call: an in-place edit through torch is narrowed and
    range-checked again (into a new copy: a plan built on the old one is no longer found, _check_index_version).  The
    entry holds the source tensor weakly and goes away with it; the copy then lives on only inside a plan built on it.
    The kernels take int32 indices only.
    SpMV and SpMM operands only (what the slot's type list admits and this backend does not)."""
    csr = isinstance(a, csr_view)
    idx = a.colind() if csr else a.rowind()
    if idx is None or idx.dtype != torch.int64:
        return a
    if a.values() is not None and a.values().dtype in _COMPLEX:
        raise TypeError(f"{what}: complex values take int32 column indices only")
    if a.values() is not None and a.values().dtype in _LOWP:
        raise TypeError(f"{what}: {a.values().dtype} values take int32 column indices only")
    key, version = id(idx), _index_version(idx)
    bound = int(a.shape()[1] if csr else a.shape()[0])     # what the copy was range-checked against is part of its identity
    hit = _NARROWED.get(key)
    if hit is None or hit[0]() is not idx or version is None or hit[1] != (version, bound, a.size()):
        dst = torch.empty(idx.numel(), dtype=torch.int32, device=idx.device)
        hd = _Handle.current(idx.device)
        rc = _capi.lib().spblas_gfx950_narrow_indices(hd.h, a.size(), _ptr(idx), _ptr(dst), bound)
        if rc == _capi.INVALID_VALUE:
            _NARROWED.pop(key, None)
            raise ValueError(f"{what}: a 64-bit index lies outside the matrix (or beyond 2^31 - 1)")
        check(rc, what)

        def forget(ref, key=key):
            # (runs on whichever thread drops the last reference: the entry is removed only if it is still THIS tensor's)
            with _NARROWED_LOCK:
                if key in _NARROWED and _NARROWED[key][0] is ref:
                    del _NARROWED[key]

        with _NARROWED_LOCK:
            hit = _NARROWED[key] = (weakref.ref(idx, forget), (version, bound, a.size()), dst)
    if csr:
        return csr_view(a.values(), a.rowptr(), hit[2], a.shape(), a.size())
    return csc_view(a.values(), a.colptr(), hit[2], a.shape(), a.size())


def _wide_indices(a_base):
    idx = a_base.colind() if isinstance(a_base, csr_view) else a_base.rowind() if isinstance(a_base, csc_view) else None
    return idx if idx is not None and idx.dtype == torch.int64 else None


def _note_index_version(state, a_base):
    """multiply_inspect on an operand with int64 indices: remember which contents of the index tensor the plan was built on."""
    idx = _wide_indices(a_base)
    if idx is not None and state is not None:
        state.index_src = (weakref.ref(idx), _index_version(idx))


def _check_index_version(info, a, a_base):
    """The plan binds the structure (like the reference's inspect): int64 indices edited in place after multiply_inspect
    are a user error, and one this layer can see -- it raises instead of multiplying with the old structure."""
    idx = _wide_indices(a_base)
    if idx is None:
        return
    mo = _get_matrix_opt(a)
    for state in (info.state_ if info is not None else None, mo._plan if mo is not None else None):
        src = getattr(state, "index_src", None)
        if src is not None and src[0]() is idx and src[1] != _index_version(idx):
            raise ValueError("multiply: the 64-bit index array was modified in place after multiply_inspect; "
                             "inspect the matrix again (a plan is tied to the structure it was built on)")


def _check_csr(a, what):
    if a.colind() is not None and a.colind().dtype != torch.int32:
        raise TypeError(f"{what}: column indices must be int32 (spblas::index_t on GPU backends; SpMV / SpMM also take int64)")
    if a.rowptr().dtype not in _OT:
        raise TypeError(f"{what}: row offsets must be int32 or int64")
    for t in (a.values(), a.rowptr(), a.colind()):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{what}: arrays must be contiguous")


def _reject_conjugated(*ts):
    if any(is_conjugated(t) for t in ts):
        raise RuntimeError("gfx950 backend does not support conjugated views.")  # spmv_impl.hpp:29-33


def _plan_key(a_base):
    """Identity of a plan = the structure arrays (the library's own check, csrc/spmv.hip); the value array may
    be rebound or change between multiplies like in the reference, where inspect holds no values at all."""
    return (a_base.rowptr().data_ptr(), a_base.colind().data_ptr(), tuple(a_base.shape()), a_base.size(),
            a_base.rowptr().dtype, a_base.values().dtype)


def _build_plan(a_base, alg=_capi.SPMV_AUTO, snapshot=0):
    """snapshot: the value of SPBLAS_GFX950_OPT_VALUE_SNAPSHOT -- 1 / True: AUTO may choose the plan that keeps a re-tiled
    copy of the values (matrix_opt operands); 2: and the plan keeps its source positions from the start."""
    hd = _Handle.current(a_base.rowptr().device)
    vt, _ = _vtype(a_base.values(), "multiply_inspect", complex_ok=True, lowp_ok=True)
    plan = ctypes.c_void_p()
    m, n = a_base.shape()
    hd.set_option(_capi.OPT_VALUE_SNAPSHOT, int(snapshot))
    try:
        check(_capi.lib().spblas_gfx950_spmv_plan_create(hd.h, ctypes.byref(plan), m, n, a_base.size(),
                                                         _ptr(a_base.rowptr()), _ptr(a_base.colind()),
                                                         _ptr(a_base.values()), _OT[a_base.rowptr().dtype], vt, alg),
              "multiply_inspect")
    finally:
        hd.set_option(_capi.OPT_VALUE_SNAPSHOT, 0)
    return _Plan(hd, plan, _plan_key(a_base), (a_base.rowptr(), a_base.colind(), a_base.values()))


class _CscPlan:
    """multiply_inspect on a csc_view / transposed(csr) operand: the operand is materialised once as
    row-major CSR on the device (spblas_gfx950_csr_transpose: stable counting sort, the device
    counterpart of algorithms/transpose_impl.hpp:14-53) and planned like any CSR matrix, so the
    execute phase runs the regular kernels instead of the atomic scatter.  Holds a snapshot of the
    values (inspect may re-format the matrix, README.md:27-30)."""

    def __init__(self, a_csc, alg):
        self.key = _csc_key(a_csc)
        self.stamp = _values_stamp(a_csc.values())
        m, n = a_csc.shape()          # logical shape of the operand
        nnz = a_csc.size()
        dev, vals = a_csc.values().device, a_csc.values()
        # the device transpose takes 32-bit offsets; 64-bit ones that fit are narrowed once into a plan-owned copy
        # (multiply_inspect leaves operands with more than 2^31 - 1 entries to the plan-free kernels)
        self.colptr32 = a_csc.colptr() if a_csc.colptr().dtype == torch.int32 else a_csc.colptr().to(torch.int32)
        self.rowptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
        self.colind = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        self.values = torch.empty(max(nnz, 1), dtype=vals.dtype, device=dev)
        hd = _Handle.current(dev)
        # the stored arrays are the CSR of the (n x m) transpose
        check(_capi.lib().spblas_gfx950_csr_transpose(hd.h, n, m, nnz, _ptr(self.colptr32), _ptr(a_csc.rowind()),
                                                      _ptr(vals), _ptr(self.rowptr), _ptr(self.colind),
                                                      _ptr(self.values), _vtype(vals, "multiply_inspect")[0]),
              "multiply_inspect")
        self.a_csr = csr_view(self.values[:nnz], self.rowptr, self.colind[:nnz], (m, n), nnz)
        self.plan = _build_plan(self.a_csr, alg, snapshot=True)  # the materialised form is a copy anyway
        # a self-contained plan (tiles with their own values, no hub rows, no hot split) needs the materialised arrays no
        # longer: they are released, and the inspected operand holds the plan alone (cfg2-sized: 1.43 instead of 2.43 x the
        # matrix).  SpMM plans and every other SpMV plan keep them.
        self.detached = False
        self._alg, self._vtype = alg, _vtype(vals, "multiply_inspect")[0]
        if alg != _capi.SPMV_ROWBLOCK and alg != _capi.SPMV_VECTOR and \
                _capi.lib().spblas_gfx950_spmv_plan_detach(hd.h, self.plan.plan) == _capi.SUCCESS:
            self.detached = True
            self.plan.tensors = None
            self.a_csr = self.rowptr = self.colind = self.values = None

    def refresh_if_stale(self, a_csc):
        """The operand's values were rebound or changed in place (torch / scale()) since inspect: transpose
        again into the same arrays (the structure is unchanged, so the plan stays valid) and refresh the plan's
        own copy, so that multiply reads current values like the reference (multiply_impl.hpp:48-52)."""
        if _values_stamp(a_csc.values()) == self.stamp:
            return
        if self.detached:  # (the arrays the plan could be refreshed from are gone: materialise and plan again)
            self.__init__(a_csc, self._alg)
            return
        m, n = a_csc.shape()
        nnz = a_csc.size()
        hd = _Handle.current(a_csc.values().device)
        check(_capi.lib().spblas_gfx950_csr_transpose(hd.h, n, m, nnz, _ptr(self.colptr32), _ptr(a_csc.rowind()),
                                                      _ptr(a_csc.values()), _ptr(self.rowptr), _ptr(self.colind),
                                                      _ptr(self.values), _vtype(a_csc.values(), "multiply")[0]),
              "multiply")
        self.stamp = _values_stamp(a_csc.values())
        self.key = _csc_key(a_csc)
        if self.plan.snapshot:
            self.plan.update_values(self.a_csr.values())

    def info(self):
        return self.plan.info()

    def held_bytes(self):
        """device bytes of the materialised row-major copy this plan holds next to the CSR plan's own (info()['device_bytes'])"""
        t = [self.rowptr, self.colind, self.values]
        return sum(x.numel() * x.element_size() for x in t if x is not None)


def _csc_key(a_csc):
    return (a_csc.colptr().data_ptr(), a_csc.rowind().data_ptr(), tuple(a_csc.shape()), a_csc.size(),
            a_csc.values().dtype)


def transpose_inspect(a, b):
    """transpose_inspect(a, b) (algorithms/transpose_impl.hpp:9-12): nothing to prepare."""
    return operation_info_t()


def transpose(*args):
    """transpose(a, b) / transpose(info, a, b): b = a^T for csr_view operands on the device, entries
    of every output row in source order exactly like the reference's counting sort
    (algorithms/transpose_impl.hpp:14-53).  b's arrays are caller-allocated."""
    a, b = args[-2], args[-1]
    _reject_lowp("transpose", a, b)
    if not (isinstance(a, csr_view) and isinstance(b, csr_view)):
        raise TypeError("transpose: csr_view operands")
    if a.shape()[0] != b.shape()[1] or a.shape()[1] != b.shape()[0]:
        raise ValueError("transpose: matrix dimensions are incompatible.")  # transpose_impl.hpp:17-21
    nnz = a.size()
    if b.values() is None or b.colind() is None or b.values().numel() < nnz or b.colind().numel() < nnz:
        raise RuntimeError("transpose: Transpose ran out of memory.")  # transpose_impl.hpp:22-25
    _check_csr(a, "transpose")
    # the device kernel works on 32-bit offsets (its positions are 32-bit: nnz <= 2^31 - 1, checked there); 64-bit
    # offset arrays -- csr_view is templated on the offset type, views/csr_view.hpp -- are narrowed on the way in and
    # widened on the way out
    if nnz >= 2 ** 31:
        raise ValueError("transpose: more than 2^31 - 1 stored entries are not supported on the device")
    a_rp = a.rowptr() if a.rowptr().dtype == torch.int32 else a.rowptr().to(torch.int32)
    b_rp = b.rowptr() if b.rowptr().dtype == torch.int32 else torch.empty(b.shape()[0] + 1, dtype=torch.int32,
                                                                          device=b.rowptr().device)
    hd = _Handle.current(a.rowptr().device)
    check(_capi.lib().spblas_gfx950_csr_transpose(hd.h, a.shape()[0], a.shape()[1], nnz, _ptr(a_rp),
                                                  _ptr(a.colind()), _ptr(a.values()), _ptr(b_rp),
                                                  _ptr(b.colind()), _ptr(b.values()),
                                                  _vtype(a.values(), "transpose")[0]), "transpose")
    if b_rp is not b.rowptr():
        b.rowptr()[:b.shape()[0] + 1].copy_(b_rp)
    _note_write(b.values(), b.colind())
    b.update(b.values(), b.rowptr(), b.colind(), b.shape(), nnz)  # transpose_impl.hpp:54


def scale(alpha, t):
    """scale(alpha, t) (algorithms/scale_impl.hpp:13-31): multiplies the stored values of a matrix view, or the
    elements of a dense vector, by alpha in place on the device.  An LDS-sliced SpMV plan of the matrix holds
    a snapshot of the values: call update_values on it afterwards."""
    base = get_ultimate_base(t)
    vals = base if _is_tensor(base) else base.values()
    if vals is None or not vals.is_contiguous():
        raise ValueError("scale: the values must be a contiguous device array")
    nvals = vals.numel() if _is_tensor(base) else base.size()
    vt, ct = _vtype(vals, "scale")
    a = ct(alpha)
    hd = _Handle.current(vals.device)
    check(_capi.lib().spblas_gfx950_scale(hd.h, nvals, ctypes.byref(a), _ptr(vals), vt), "scale")
    if not _is_tensor(base):  # plans holding a copy of these values see the change (_Plan.refresh_if_stale)
        _note_write(vals)


def _find_plan(info, a, a_base):
    key = _plan_key(a_base)
    if info is not None and isinstance(info.state_, _Plan) and info.state_.key == key:
        return info.state_
    mo = _get_matrix_opt(a)
    if mo is not None and isinstance(mo._plan, _Plan) and mo._plan.key == key:
        return mo._plan
    return None


# --------------------------------------------------------------------------- SpMV / SpMM
def _spmv(info, a, b, c, prepare_only=False):
    if _is_complex_view(a) or _is_complex_view(b):
        return _spmv_complex(info, a, b, c, prepare_only)
    if _lowp_dtype(a) or _lowp_dtype(b):
        return _spmv_lowp(info, a, b, c, prepare_only)
    a_base, b_base = get_ultimate_base(a), get_ultimate_base(b)
    _check_index_version(info, a, a_base)
    a_base = _int32_columns(a_base, "multiply")
    _reject_conjugated(a, b, c)
    if not _is_tensor(c) or c.dim() != 1:
        raise TypeError("multiply: the output vector must be a plain 1-D device tensor")
    op = _capi.OP_N
    csc_plan = None
    if isinstance(a_base, csc_view):
        if info is not None and isinstance(info.state_, _CscPlan) and info.state_.key == _csc_key(a_base):
            csc_plan = info.state_       # inspected: regular kernels on the materialised CSR
            csc_plan.refresh_if_stale(a_base)
            a_csr = csc_plan.a_csr
        else:
            # CSC = CSR of the transpose + TRANSPOSE (vendor/rocsparse/detail/get_transpose.hpp:19-29)
            a_csr = csr_view(a_base.values(), a_base.colptr(), a_base.rowind(),
                             (a_base.shape()[1], a_base.shape()[0]), a_base.size())
            op = _capi.OP_T
    else:
        a_csr = a_base
    detached = csc_plan is not None and csc_plan.detached
    if not detached:
        _check_csr(a_csr, "multiply")
    if a_base.shape()[0] != c.shape[0] or a_base.shape()[1] != b_base.shape[0]:
        # algorithms/multiply_impl.hpp:37-41
        raise ValueError("multiply: matrix and vector dimensions are incompatible.")
    vt, ct = _vtype(a_base.values() if detached else a_csr.values(), "multiply")
    if b_base.dtype != a_base.values().dtype or c.dtype != a_base.values().dtype:
        raise TypeError("multiply: A, x and y must share one value type")
    if not (b_base.is_contiguous() and c.is_contiguous()):
        raise ValueError("multiply: x and y must be contiguous")
    alpha_opt = get_scaling_factor(a, b)
    alpha = ct(1 if alpha_opt is None else alpha_opt)  # spmv_impl.hpp:35-37
    beta = ct(0)
    hd = _Handle.current(c.device)
    plan = csc_plan.plan if csc_plan else (_find_plan(info, a, a_base) if op == _capi.OP_N else None)
    if plan is not None and not csc_plan:
        plan.refresh_if_stale(a_csr.values())
    if detached:  # the plan is all there is of the materialised operand: no matrix arrays in the call
        m, n = a_base.shape()
        args = (hd.h, plan.plan, op, m, n, a_base.size(), ctypes.byref(alpha), None, None, None, _ptr(b_base),
                ctypes.byref(beta), _ptr(c), _capi.I32, vt)
    else:
        m, n = a_csr.shape()
        args = (hd.h, plan.plan if plan else None, op, m, n, a_csr.size(), ctypes.byref(alpha), _ptr(a_csr.rowptr()),
                _ptr(a_csr.colind()), _ptr(a_csr.values()), _ptr(b_base), ctypes.byref(beta), _ptr(c),
                _OT[a_csr.rowptr().dtype], vt)
    if prepare_only:  # the entry point with its bound arguments; keep the operands alive with the bound call
        # (a_csr: with int64 indices it holds the narrowed int32 copy the bound pointers refer to)
        return (_capi.lib().spblas_gfx950_spmv, args), (alpha, beta, plan, a, b, c, a_csr)
    check(_capi.lib().spblas_gfx950_spmv(*args), "multiply")


class prepared_multiply:
    """multiply(info, a, x, y) validated and bound ONCE; calling the object re-issues the same
    SpMV on the stream that was current at construction (the handle is put back on that stream before every
    launch: other API calls re-bind it to whatever stream is current when they run).  For solver-style loops
    where the Python host layer (view unwrapping, checks: tens of microseconds) would otherwise cost more than the
    kernel.  The operands must stay the same tensors; their contents may change between calls.  A plan carries
    workspaces and must not run on two streams at once."""

    def __init__(self, info, a, x, y):
        (self._fn, self._args), self._keep = _spmv(info, a, x, y, prepare_only=True)
        self._set_stream = _capi.lib().spblas_gfx950_set_stream
        self._stream = ctypes.c_void_p(torch.cuda.current_stream(y.device).cuda_stream)
        a_base = get_ultimate_base(a)
        self._plan = self._keep[2]
        self._values = a_base.values() if isinstance(a_base, csr_view) else None

    def __call__(self):
        if self._plan is not None and self._plan.snapshot and self._values is not None:
            self._plan.refresh_if_stale(self._values)
        self._set_stream(self._args[0], self._stream)
        rc = self._fn(*self._args)
        if rc:
            check(rc, "multiply")


def _spmm(info, a, b, c):
    if _is_complex_view(a) or _is_complex_view(b):
        return _spmm_complex(info, a, b, c)
    if _lowp_dtype(a) or _lowp_dtype(b):
        return _spmm_lowp(info, a, b, c)
    a_base, b_base = get_ultimate_base(a), get_ultimate_base(b)
    _check_index_version(info, a, a_base)
    a_base = _int32_columns(a_base, "multiply")
    _reject_conjugated(a, b, c)
    plan = None
    if isinstance(a_base, csc_view):
        # CSC operand (test/gtest/spmm_test.cpp:181): run the CSR kernel on the materialised row-major
        # form -- taken from the inspect result when there is one, otherwise transposed for this call
        if info is not None and isinstance(info.state_, _CscPlan) and info.state_.key == _csc_key(a_base) and \
                not info.state_.detached:  # (a plan inspected for SpMV may have released its row-major arrays)
            info.state_.refresh_if_stale(a_base)
            plan = info.state_.plan
            a_base = info.state_.a_csr
        else:
            a_base = _CscPlan(a_base, _capi.SPMV_VECTOR).a_csr
    elif isinstance(a_base, csr_view):
        plan = _find_plan(info, a, a_base)  # what multiply_inspect(a, B, C) left in info / in the matrix_opt
    if not isinstance(a_base, csr_view):
        raise NotImplementedError("gfx950 SpMM: A must have a csr_view or csc_view base")
    if not _is_tensor(c) or c.dim() != 2:
        raise TypeError("multiply: the output matrix must be a plain 2-D row-major device tensor")
    _check_csr(a_base, "multiply")
    if (a_base.shape()[0] != c.shape[0] or b_base.shape[1] != c.shape[1]
            or a_base.shape()[1] != b_base.shape[0]):
        raise ValueError("multiply: matrix dimensions are incompatible.")  # multiply_impl.hpp:70-76
    vt, ct = _vtype(a_base.values(), "multiply")
    if b_base.dtype != a_base.values().dtype or c.dtype != a_base.values().dtype:
        raise TypeError("multiply: A, B and C must share one value type")
    # Dense operands: layout_right (row-major) or layout_left (column-major, mdspan_col_major of detail/mdspan.hpp:31-36) --
    # the reference's CPU path takes any layout through mdspan's operator() (backend/view_customizations.hpp:230-240).
    # Anything else (overlapping or doubly strided views) is refused like a non-mdspan argument would be.
    m, k = a_base.shape()
    n = c.shape[1]

    (brs, bcs), (crs, ccs) = _dense_strides(b_base, k, n), _dense_strides(c, m, n)
    alpha_opt = get_scaling_factor(a, b)
    alpha, beta = ct(1 if alpha_opt is None else alpha_opt), ct(0)
    hd = _Handle.current(c.device)
    check(_capi.lib().spblas_gfx950_spmm_strided(hd.h, plan.plan if plan is not None else None, m, k, n, a_base.size(),
                                                 ctypes.byref(alpha),
                                                 _ptr(a_base.rowptr()), _ptr(a_base.colind()), _ptr(a_base.values()),
                                                 _ptr(b_base), brs, bcs, ctypes.byref(beta), _ptr(c), crs, ccs,
                                                 _OT[a_base.rowptr().dtype], vt), "multiply")


def _is_sparse(t):
    return isinstance(get_ultimate_base(t), (csr_view, csc_view))


def _leading_info(args, n, names):
    """args = the n operands `names`, with or without an info in front -> (info or None, the operands)."""
    if len(args) == n + 1:
        return args[0], args[1:]
    if len(args) == n:
        return None, args
    raise TypeError(f"expected ({names}) or (info, {names})")


def multiply(*args):
    """multiply(a, b, c) / multiply(info, a, b, c): c = a * b.
    SpMV when b is a vector, SpMM when b is a dense matrix
    (vendor/rocsparse/detail/spmv_impl.hpp:25,87; vendor/onemkl_sycl/spmm_impl.hpp:96-125)."""
    info, (a, b, c) = _leading_info(args, 3, "a, b, c")
    b_base = get_ultimate_base(b)
    if isinstance(info, spgemm_state_t) or _is_sparse(b):
        raise TypeError("SpGEMM is two-phase on device backends: use multiply_compute + multiply_fill")
    if not _is_tensor(b_base):
        raise TypeError("multiply: b must be a device tensor (vector or row-major matrix)")
    if b_base.dim() == 1:
        return _spmv(info, a, b, c)
    return _spmm(info, a, b, c)


def multiply_inspect(*args, alg=_capi.SPMV_AUTO, values_will_change=False):
    """multiply_inspect(a, b, c) -> operation_info_t, or multiply_inspect(info, a, b, c).
    Builds the gfx950 row partition on device and stores it in the info's state_; when A
    is wrapped in matrix_opt it is cached there too (the oneMKL model,
    vendor/onemkl_sycl/spmm_impl.hpp:48-61, views/matrix_opt_impl.hpp:90-92).

    Values: for a plain csr_view the plan holds structure only and every multiply reads a.values() as the
    reference does (algorithms/multiply_impl.hpp:48-52).  Wrapping A in matrix_opt -- "this view owns an
    optimised form of the matrix" -- additionally lets AUTO pick the LDS-sliced plan, which re-tiles A and
    multiplies with its own copy of the values (5x faster when x misses every cache).  The copy is refreshed
    automatically when a.values() is rebound, modified in place through torch, or scaled with scale();
    after writing it with a kernel of your own call info.state_.update_values(values).  alg=SPMV_SLICED asks
    for that plan explicitly, with the same contract.  values_will_change=True (a time-stepping caller) makes such a plan
    keep the source position of every entry from the start (+4 B per entry): the first refresh is then a gather like every
    later one instead of a second inspect (SPBLAS_GFX950_OPT_VALUE_SNAPSHOT = 2)."""
    info, (a, b, c) = _leading_info(args, 3, "a, b, c")
    ret = info is None
    if info is None:
        info = operation_info_t()
    if isinstance(info, spgemm_state_t):
        return None  # vendor/rocsparse/multiply_spgemm.hpp:232-235: no-op
    a_base = get_ultimate_base(a)
    if _is_complex_view(a) and not _is_sparse(b):  # conjugated complex operands are taken (csr_view only)
        a_base = _complex_operand(a, "multiply_inspect")
    elif _lowp_dtype(a) and not _is_sparse(b):  # 16-bit: csr_view with int32 columns only
        a_base = _lowp_operand(a, "multiply_inspect")
        _reject_conjugated(a, b, c)
    else:
        _reject_conjugated(a, b, c)
    wide_base = a_base
    if isinstance(a_base, (csr_view, csc_view)) and not _is_sparse(b) and a_base.values() is not None:
        a_base = _int32_columns(a_base, "multiply_inspect")
    if isinstance(a_base, csr_view) and not _is_sparse(b) and a_base.values() is not None:
        _check_csr(a_base, "multiply_inspect")
        # the column-sliced plan serves SpMV only; SpMM uses the row partition (spmm_impl.hpp of the C++ layer)
        b_base = get_ultimate_base(b)
        is_spmm = _is_tensor(b_base) and b_base.dim() == 2
        mo = _get_matrix_opt(a)
        plan = _build_plan(a_base, _capi.SPMV_ROWBLOCK if is_spmm and alg == _capi.SPMV_AUTO else alg,
                           snapshot=0 if mo is None and alg != _capi.SPMV_SLICED else (2 if values_will_change else 1))
        if is_spmm:
            plan.spmm_inspect()
        info.state_ = plan
        _note_index_version(plan, wide_base)
        if mo is not None:
            mo._plan = plan
    elif isinstance(a_base, csc_view) and _is_tensor(get_ultimate_base(b)) and a_base.size() < 2 ** 31:
        is_spmm = get_ultimate_base(b).dim() == 2
        info.state_ = _CscPlan(a_base, _capi.SPMV_ROWBLOCK if is_spmm else alg)
        if is_spmm:
            info.state_.plan.spmm_inspect()
        _note_index_version(info.state_, wide_base)
    return info if ret else None


# --------------------------------------------------------------------------- SpGEMM
def _device_transposed(x):
    """csr_view of x^T in freshly allocated device arrays (spblas_gfx950_csr_transpose)."""
    m, n = x.shape()
    nnz = x.size()
    dev = x.rowptr().device
    t = csr_view(torch.empty(nnz, dtype=x.values().dtype, device=dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                 torch.empty(nnz, dtype=torch.int32, device=dev), (n, m), nnz)
    transpose(x, t)
    return t


def _csr_form(t_base, want_transposed, what):
    """CSR arrays of X (or of X^T) for a csr_view / csc_view X.  A csc_view's arrays ARE the CSR arrays of
    X^T (algorithms/transposed.hpp:7-21), so only one of the two forms needs the device transpose."""
    if isinstance(t_base, csc_view):
        t_base, want_transposed = transposed(t_base), not want_transposed
    if not isinstance(t_base, csr_view):
        raise NotImplementedError("gfx950 SpGEMM operands must have a csr_view or csc_view base")
    _check_csr(t_base, what)
    if t_base.rowptr().dtype != torch.int32:
        raise TypeError("SpGEMM: int32 row offsets only")
    return _device_transposed(t_base) if want_transposed else t_base


def _spgemm_operands(a, b, c, d=None):
    """Operands of the CSR kernel for any mix of csr_view / csc_view A, B, C (the eight combinations of
    algorithms/detail/spgemm/spgemm_{gustavsons,innerproduct,outerproduct}.hpp): with a CSR result the
    kernel runs on CSR(A), CSR(B); with a CSC result it computes C^T = B^T A^T, whose CSR arrays are C's CSC
    arrays.  Operands stored the other way round are transposed on the device for this call.
    Returns (a_eff, b_eff, c_eff, d_eff)."""
    a_base, b_base = get_ultimate_base(a), get_ultimate_base(b)
    _reject_complex("multiply_compute", a, b, c, d)
    _reject_lowp("multiply_compute", a, b, c, d)
    if not isinstance(c, (csr_view, csc_view)):
        raise NotImplementedError("gfx950 SpGEMM result must be a csr_view or csc_view")
    _reject_conjugated(a, b)
    if (_shape_of(a_base)[0] != c.shape()[0] or _shape_of(b_base)[1] != c.shape()[1]
            or _shape_of(a_base)[1] != _shape_of(b_base)[0]):
        raise ValueError("multiply: matrix dimensions are incompatible.")  # spgemm_gustavsons.hpp:22-27
    d_base = None
    if d is not None:
        d_base = get_ultimate_base(d)
        _reject_conjugated(d)
        if tuple(_shape_of(d_base)) != tuple(c.shape()):
            raise ValueError("multiply: matrix dimensions are incompatible.")
    if isinstance(c, csr_view):
        return (_csr_form(a_base, False, "multiply_compute"), _csr_form(b_base, False, "multiply_compute"), c,
                None if d_base is None else _csr_form(d_base, False, "multiply_compute"))
    c_eff = csr_view(c.values(), c.colptr(), c.rowind(), (c.shape()[1], c.shape()[0]), c.size())
    return (_csr_form(b_base, True, "multiply_compute"), _csr_form(a_base, True, "multiply_compute"), c_eff,
            None if d_base is None else _csr_form(d_base, True, "multiply_compute"))


def _symbolic(state, a, b, c_user, d=None):
    a_base, b_base, c, d_base = _spgemm_operands(a, b, c_user, d)
    if c.rowptr() is None or c.rowptr().dtype != torch.int32 or c.rowptr().numel() < c.shape()[0] + 1:
        raise ValueError("multiply_compute: c's offsets must hold shape+1 int32 entries")
    hd, st = state._ensure(c.rowptr().device)
    state._keep = (a_base, b_base, d_base)  # device transposes of this call stay alive with the state
    nnz = ctypes.c_int64(0)
    m, k = a_base.shape()
    n = b_base.shape()[1]
    if d is not None:
        check(_capi.lib().spblas_gfx950_spgemm_set_addend(hd.h, st, d_base.size(), _ptr(d_base.rowptr()),
                                                          _ptr(d_base.colind())), "multiply_compute")
    else:
        check(_capi.lib().spblas_gfx950_spgemm_set_addend(hd.h, st, 0, None, None), "multiply_compute")
    state._has_addend = d is not None
    check(_capi.lib().spblas_gfx950_spgemm_symbolic(hd.h, st, m, k, n, a_base.size(), _ptr(a_base.rowptr()),
                                                    _ptr(a_base.colind()), b_base.size(), _ptr(b_base.rowptr()),
                                                    _ptr(b_base.colind()), _ptr(c.rowptr()), ctypes.byref(nnz)),
          "multiply_compute")
    state._result_shape, state._result_nnz = index(c_user.shape()), nnz.value
    state._last_colind = None


def _numeric(state, a, b, c_user, d=None):
    a_base, b_base, c, d_base = _spgemm_operands(a, b, c_user, d)
    if state._state is None:
        raise RuntimeError("multiply_fill: multiply_compute has not been called on this state")
    if (d is not None) != getattr(state, "_has_addend", False):
        raise RuntimeError("multiply_fill: the addend must be passed to both multiply_compute and multiply_fill")
    hd, st = state._ensure(c.rowptr().device)
    state._keep = (a_base, b_base, d_base)
    nnz = state._result_nnz
    cap = 0
    if c.values() is not None and c.colind() is not None:
        cap = min(c.values().numel(), c.colind().numel())
    if cap < nnz:
        raise RuntimeError("multiply: SpGEMM ran out of memory.")  # spgemm_gustavsons.hpp:44-48
    vt, ct = _vtype(a_base.values(), "multiply_fill")
    alpha_opt = get_scaling_factor(a, b)
    alpha = ct(1 if alpha_opt is None else alpha_opt)
    if d is not None:
        if d_base.values().dtype != a_base.values().dtype:
            raise TypeError("multiply_fill: the addend must have A's value type")
        beta_opt = get_scaling_factor(d)
        beta = ct(1 if beta_opt is None else beta_opt)  # multiply_spgemm.hpp:188-189
        check(_capi.lib().spblas_gfx950_spgemm_numeric_addend(
            hd.h, st, ctypes.byref(alpha), _ptr(a_base.rowptr()), _ptr(a_base.colind()), _ptr(a_base.values()),
            _ptr(b_base.rowptr()), _ptr(b_base.colind()), _ptr(b_base.values()), ctypes.byref(beta),
            _ptr(d_base.rowptr()), _ptr(d_base.colind()), _ptr(d_base.values()), _ptr(c.rowptr()),
            _ptr(c.colind()), _ptr(c.values()), cap, vt), "multiply_fill")
        _note_write(c.values(), c.colind())
    else:
        # Repeated fills of ONE result may leave its column indices alone (OPT_SPGEMM_KEEP_COLIND) -- but only when
        # this is provably the array the previous fill wrote and nobody touched it since: the same tensor object
        # (which this state keeps alive, so its address cannot have been recycled) with an unchanged version counter.
        # Writes made through this library's own kernels (another state filling the same arrays, add, transpose)
        # do not move torch's counter; the module-level write epoch of the address covers those.
        ci = c.colind()
        last = getattr(state, "_last_colind", None)
        keep = last is not None and last[0] is ci and last[1] == ci._version and last[2] == ci.data_ptr() and \
            last[3] == _value_epochs.get(ci.data_ptr(), 0)
        if keep:
            hd.set_option(_capi.OPT_SPGEMM_KEEP_COLIND, 1)
        try:
            check(_capi.lib().spblas_gfx950_spgemm_numeric(hd.h, st, ctypes.byref(alpha), _ptr(a_base.rowptr()),
                                                           _ptr(a_base.colind()), _ptr(a_base.values()),
                                                           _ptr(b_base.rowptr()), _ptr(b_base.colind()),
                                                           _ptr(b_base.values()), _ptr(c.rowptr()), _ptr(ci),
                                                           _ptr(c.values()), cap, vt), "multiply_fill")
        finally:
            if keep:
                hd.set_option(_capi.OPT_SPGEMM_KEEP_COLIND, 0)
        _note_write(c.values())
        if not keep:
            _note_write(ci)
        state._last_colind = (ci, ci._version, ci.data_ptr(), _value_epochs.get(ci.data_ptr(), 0))
    if isinstance(c_user, csr_view):
        c_user.update(c.values(), c.rowptr(), c.colind(), state._result_shape, nnz)  # spgemm_gustavsons.hpp:50-51
    else:
        c_user.update(c.values(), c.rowptr(), c.colind(), state._result_shape, nnz)  # the CSR arrays of C^T


def multiply_compute(*args):
    """multiply_compute(a, b, c) -> operation_info_t; multiply_compute(info, a, b, c);
    multiply_compute(spgemm_state, a, b, c)   (algorithms/multiply.hpp:48-52,
    vendor/rocsparse/multiply_spgemm.hpp:72-118,277-283).  Writes c.rowptr, reports nnz(C)."""
    if len(args) == 5:  # (spgemm_state, a, b, c, d): C = alpha*A*B + beta*D, multiply_spgemm.hpp:237-243
        if not isinstance(args[0], spgemm_state_t):
            raise TypeError("multiply_compute(state, a, b, c, d): the five-argument form takes a spgemm_state_t")
        return _symbolic(*args)
    info, (a, b, c) = _leading_info(args, 3, "a, b, c")
    if isinstance(info, spgemm_state_t):
        return _symbolic(info, a, b, c)
    ret = info is None
    if info is None:
        info = operation_info_t()
    if not isinstance(info.state_, spgemm_state_t):
        info.state_ = spgemm_state_t()
    _symbolic(info.state_, a, b, c)
    info.update_impl_(info.state_.result_shape(), info.state_.result_nnz())
    return info if ret else None


def multiply_fill(info, a, b, c, d=None):
    """multiply_fill(info | spgemm_state, a, b, c[, d]) (algorithms/multiply.hpp:54-55,
    vendor/rocsparse/multiply_spgemm.hpp:123-145,245-250)."""
    state = info if isinstance(info, spgemm_state_t) else info.state_
    if not isinstance(state, spgemm_state_t):
        raise RuntimeError("multiply_fill: info does not come from multiply_compute")
    return _numeric(state, a, b, c, d)


# symbolic/numeric reuse family (vendor/rocsparse/multiply_spgemm.hpp:252-274,293-317)
def multiply_symbolic_compute(state, a, b, c, d=None):
    return _symbolic(state, a, b, c, d)


def multiply_symbolic_fill(state, a, b, c, d=None):
    """Leaves the STRUCTURE of C (rowptr and colind) in the caller's arrays, as the reference's symbolic stage does
    (vendor/rocsparse/multiply_spgemm.hpp:147-176; test/gtest/device/spgemm_reuse_test.cpp:325-400 copies those arrays
    afterwards and hands the copies to multiply_numeric).  The column indices come out of the same pass as the values
    here, so this is one numeric pass."""
    if state._state is None:
        raise RuntimeError("multiply_symbolic_fill: multiply_symbolic_compute has not been called")
    return _numeric(state, a, b, c, d)


def multiply_numeric(state, a, b, c, d=None):
    return _numeric(state, a, b, c, d)


# --------------------------------------------------------------------------- add
def _add_operands(a, b, c):
    a_base, b_base = get_ultimate_base(a), get_ultimate_base(b)
    _reject_complex("add", a, b, c)
    _reject_lowp("add", a, b, c)
    if not (isinstance(a_base, csr_view) and isinstance(b_base, csr_view) and isinstance(c, csr_view)):
        raise NotImplementedError("gfx950 add supports CSR + CSR -> CSR")
    _reject_conjugated(a, b)
    for t in (a_base, b_base):
        _check_csr(t, "add")
        if t.rowptr().dtype != torch.int32:
            raise TypeError("add: int32 row offsets only")
    if tuple(a_base.shape()) != tuple(b_base.shape()) or tuple(b_base.shape()) != tuple(c.shape()):
        raise ValueError("add: matrix dimensions are incompatible.")  # add_impl.hpp:44-47,83-86
    if a_base.values().dtype != b_base.values().dtype:
        raise TypeError("add: a and b must have the same value type")
    return a_base, b_base


def _add_symbolic(state, a, b, c):
    a_base, b_base = _add_operands(a, b, c)
    if c.rowptr() is None or c.rowptr().dtype != torch.int32 or c.rowptr().numel() < c.shape()[0] + 1:
        raise ValueError("add_inspect: c.rowptr must hold shape[0]+1 int32 entries")
    hd, st = state._ensure(c.rowptr().device)
    nnz = ctypes.c_int64(0)
    m, n = a_base.shape()
    check(_capi.lib().spblas_gfx950_csr_add_symbolic(hd.h, st, m, n, a_base.size(), _ptr(a_base.rowptr()),
                                                     _ptr(a_base.colind()), b_base.size(), _ptr(b_base.rowptr()),
                                                     _ptr(b_base.colind()), _ptr(c.rowptr()), ctypes.byref(nnz)),
          "add_inspect")
    state._result_shape, state._result_nnz = index(m, n), nnz.value
    state._has_addend = True


def _add_numeric(state, a, b, c):
    a_base, b_base = _add_operands(a, b, c)
    hd, st = state._ensure(c.rowptr().device)
    nnz = state._result_nnz
    cap = 0
    if c.values() is not None and c.colind() is not None:
        cap = min(c.values().numel(), c.colind().numel())
    if cap < nnz:  # add_impl.hpp:67-72
        raise RuntimeError("add: ran out of memory.  CSR output view has insufficient memory.")
    vt, ct = _vtype(a_base.values(), "add")
    sa, sb = get_scaling_factor(a), get_scaling_factor(b)
    alpha, beta = ct(1 if sa is None else sa), ct(1 if sb is None else sb)
    check(_capi.lib().spblas_gfx950_csr_add_numeric(hd.h, st, ctypes.byref(alpha), _ptr(a_base.rowptr()),
                                                    _ptr(a_base.colind()), _ptr(a_base.values()), ctypes.byref(beta),
                                                    _ptr(b_base.rowptr()), _ptr(b_base.colind()),
                                                    _ptr(b_base.values()), _ptr(c.rowptr()), _ptr(c.colind()),
                                                    _ptr(c.values()), cap, vt), "add")
    _note_write(c.values(), c.colind())
    c.update(c.values(), c.rowptr(), c.colind(), state._result_shape, nnz)  # add_impl.hpp:75-76


def add_inspect(*args):
    """add_inspect(a, b, c) -> operation_info_t / add_inspect(info, a, b, c)
    (algorithms/add.hpp:15-19, add_impl.hpp:79-108): structural nnz of A + B; also writes c.rowptr."""
    info, (a, b, c) = _leading_info(args, 3, "a, b, c")
    ret = info is None
    if info is None:
        info = operation_info_t()
    if not isinstance(info.state_, spgemm_state_t):
        info.state_ = spgemm_state_t()
    _add_symbolic(info.state_, a, b, c)
    info.update_impl_(info.state_.result_shape(), info.state_.result_nnz())
    return info if ret else None


def add_compute(info, a, b, c):
    """add_compute(info, a, b, c) (add_impl.hpp:110-113): fill c's colind / values."""
    if not isinstance(info.state_, spgemm_state_t) or info.state_._state is None:
        raise RuntimeError("add_compute: info does not come from add_inspect")
    return _add_numeric(info.state_, a, b, c)


def add(a, b, c):
    """add(a, b, c): c = a + b for CSR operands (add_impl.hpp:40-77); c must already own enough
    room for the result (csr_builder semantics)."""
    state = spgemm_state_t()
    _add_symbolic(state, a, b, c)
    _add_numeric(state, a, b, c)


# --------------------------------------------------------------------------- SpTRSV
class upper_triangle_t:      # detail/triangular_types.hpp:5-8
    pass


class lower_triangle_t:      # detail/triangular_types.hpp:10-13
    pass


class implicit_unit_diagonal_t:  # detail/triangular_types.hpp:15-18
    pass


class explicit_diagonal_t:       # detail/triangular_types.hpp:20-23
    pass


upper_triangle, lower_triangle = upper_triangle_t(), lower_triangle_t()
implicit_unit_diagonal, explicit_diagonal = implicit_unit_diagonal_t(), explicit_diagonal_t()


class _NativePlan:
    """The state_ of a solver-side inspect: a plan of the library (destroyed with this object), the key of the arrays it was made
    for and the tensors it keeps alive.  Subclasses name their C entry points."""
    _destroy = None
    _info_call, _info_names = None, ()  # (a plan without an info entry point has no info())

    def __init__(self, hd, plan, key, tensors=None):
        self.hd, self.plan, self.key, self.tensors = hd, plan, key, tensors

    def info(self):
        arr = (ctypes.c_int64 * 4)()
        check(getattr(_capi.lib(), self._info_call)(self.plan, arr), self._info_call)
        return dict(zip(self._info_names, list(arr)))

    def __del__(self):
        try:
            if self.plan:
                getattr(_capi.lib(), self._destroy)(self.hd.h, self.plan)
                self.plan = None
        except Exception:
            pass


class _TrsvPlan(_NativePlan):
    """triangular_solve_inspect state: level sets of the dependency graph (spblas_gfx950_sptrsv_create)."""
    _destroy, _info_call = "spblas_gfx950_sptrsv_destroy", "spblas_gfx950_sptrsv_info"
    _info_names = ("levels", "max_level_width", "launches_per_solve", "lanes_per_row")

    def check_status(self):
        """Synchronises the stream; raises if a device-side wait of the last solve gave up (spblas_gfx950_sptrsv_status)."""
        st = ctypes.c_int(0)
        hd = _Handle.current(torch.device("cuda", self.hd.device))
        check(_capi.lib().spblas_gfx950_sptrsv_status(hd.h, self.plan, ctypes.byref(st)), "spblas_gfx950_sptrsv_status")
        if st.value != 0:
            raise RuntimeError("triangular_solve: a device-side wait ran into its bound; the result is not valid")


def _trsv_operands(a, uplo, diag, b, x):
    a_base = get_ultimate_base(a)
    _reject_complex("triangular_solve", a, b, x)
    _reject_lowp("triangular_solve", a, b, x)
    if not isinstance(a_base, csr_view):
        raise NotImplementedError("gfx950 triangular_solve supports csr_view operands")
    _reject_conjugated(a, b, x)
    _check_csr(a_base, "triangular_solve")
    if a_base.rowptr().dtype != torch.int32:
        raise TypeError("triangular_solve: int32 row offsets only")
    if not isinstance(uplo, (upper_triangle_t, lower_triangle_t)):
        raise TypeError("triangular_solve: uplo must be upper_triangle_t or lower_triangle_t")  # :48-49 static_assert
    if not isinstance(diag, (implicit_unit_diagonal_t, explicit_diagonal_t)):
        raise TypeError("triangular_solve: diag must be implicit_unit_diagonal_t or explicit_diagonal_t")
    if get_scaling_factor(x) is not None:
        raise NotImplementedError("gfx950 triangular_solve: x must be a plain vector")
    b = get_ultimate_base(b)  # scaled(alpha, b) is allowed (examples/simple_sptrsv.cpp:49-53): applied to x afterwards
    m, n = a_base.shape()
    # the reference asserts squareness and matching vector lengths (triangular_solve_impl.hpp:50-53); two matrices of m rows and
    # the same number of columns are a block of right-hand sides (spblas_gfx950_sptrsm_solve)
    if m != n or not _is_tensor(b) or not _is_tensor(x) or b.dim() != x.dim() or b.dim() not in (1, 2) or \
            x.shape[0] != n or b.shape[0] != m or (b.dim() == 2 and b.shape[1] != x.shape[1]):
        raise ValueError("triangular_solve: matrix and vector dimensions are incompatible.")
    if b.dtype != a_base.values().dtype or x.dtype != a_base.values().dtype:
        raise TypeError("triangular_solve: b and x must have A's value type")
    if b.dim() == 2:
        _dense_strides(b, m, b.shape[1]), _dense_strides(x, m, x.shape[1])  # row- or column-major, else ValueError
    elif not (b.is_contiguous() and x.is_contiguous()):
        raise ValueError("triangular_solve: vectors must be contiguous")
    return a_base


def _trsv_key(a_base, uplo, diag):
    return (a_base.rowptr().data_ptr(), a_base.colind().data_ptr(), tuple(a_base.shape()), a_base.size(),
            type(uplo), type(diag))


def _trsv_plan(a_base, uplo, diag):
    hd = _Handle.current(a_base.rowptr().device)
    plan = ctypes.c_void_p()
    check(_capi.lib().spblas_gfx950_sptrsv_create(
        hd.h, ctypes.byref(plan), a_base.shape()[0], a_base.size(), _ptr(a_base.rowptr()), _ptr(a_base.colind()),
        _capi.UPPER if isinstance(uplo, upper_triangle_t) else _capi.LOWER,
        _capi.DIAG_UNIT if isinstance(diag, implicit_unit_diagonal_t) else _capi.DIAG_EXPLICIT),
        "triangular_solve_inspect")
    return _TrsvPlan(hd, plan, _trsv_key(a_base, uplo, diag))


def triangular_solve_inspect(*args):
    """triangular_solve_inspect(a, uplo, diag, b, x) -> operation_info_t, or with a leading info
    (algorithms/triangular_solve.hpp:8-15).  The reference's CPU inspect is empty
    (triangular_solve_impl.hpp:13-38); here it builds the level sets the device solve needs."""
    info, (a, uplo, diag, b, x) = _leading_info(args, 5, "a, uplo, diag, b, x")
    ret = info is None
    if ret:
        info = operation_info_t()
    a_base = _trsv_operands(a, uplo, diag, b, x)
    info.state_ = _trsv_plan(a_base, uplo, diag)
    return info if ret else None


def triangular_solve(*args):
    """triangular_solve(a, uplo, diag, b, x) / triangular_solve(info, a, uplo, diag, b, x):
    x = inv(A) b using only the named triangle of A (triangular_solve_impl.hpp:41-107).  b and x may both be (m, n) tensors,
    row- or column-major (windows of wider tensors included): X(:, j) = inv(A) B(:, j) for all columns in one solve.  A plan
    made by triangular_solve_inspect with vectors serves matrices and the other way round."""
    info, (a, uplo, diag, b, x) = _leading_info(args, 5, "a, uplo, diag, b, x")
    a_base = _trsv_operands(a, uplo, diag, b, x)
    plan = info.state_ if info is not None and isinstance(info.state_, _TrsvPlan) else None
    if plan is None or plan.key != _trsv_key(a_base, uplo, diag):
        plan = _trsv_plan(a_base, uplo, diag)  # no usable inspect result: analyse now
        if info is not None:
            info.state_ = plan
    hd = _Handle.current(a_base.rowptr().device)
    vt, ct = _vtype(a_base.values(), "triangular_solve")
    sa = get_scaling_factor(a)
    alpha = ct(1 if sa is None else sa)
    sb = get_scaling_factor(b)
    bb = get_ultimate_base(b)
    if x.dim() == 2:  # a block of right-hand sides: one solve, every level handed over once for all columns
        m, n = x.shape
        (brs, bcs), (xrs, xcs) = _dense_strides(bb, m, n), _dense_strides(x, m, n)
        check(_capi.lib().spblas_gfx950_sptrsm_solve(hd.h, plan.plan, a_base.shape()[0], a_base.size(), n, ctypes.byref(alpha),
                                                     _ptr(a_base.rowptr()), _ptr(a_base.colind()), _ptr(a_base.values()),
                                                     _ptr(bb), brs, bcs, _ptr(x), xrs, xcs, vt), "triangular_solve")
        if sb is not None and x.numel() > 0:
            beta = ct(sb)
            if x.is_contiguous() or x.t().is_contiguous():
                check(_capi.lib().spblas_gfx950_scale(hd.h, x.numel(), ctypes.byref(beta), _ptr(x), vt), "triangular_solve")
            else:  # a window of a wider tensor: its lines one by one (the elements between them are not X's)
                lines = x if xcs == 1 else x.t()
                for i in range(lines.shape[0]):
                    check(_capi.lib().spblas_gfx950_scale(hd.h, lines.shape[1], ctypes.byref(beta), _ptr(lines[i]), vt),
                          "triangular_solve")
        return
    check(_capi.lib().spblas_gfx950_sptrsv_solve(hd.h, plan.plan, a_base.shape()[0], a_base.size(),
                                                 ctypes.byref(alpha), _ptr(a_base.rowptr()), _ptr(a_base.colind()),
                                                 _ptr(a_base.values()), _ptr(bb), _ptr(x), vt),
          "triangular_solve")
    if sb is not None:  # the solve is linear in b: x = inv(A) (s b) = s inv(A) b
        beta = ct(sb)
        check(_capi.lib().spblas_gfx950_scale(hd.h, x.numel(), ctypes.byref(beta), _ptr(x), vt), "triangular_solve")


def triangular_solve_sweeps(*args):
    """triangular_solve_sweeps(a, uplo, diag, b, x, sweeps) / triangular_solve_sweeps(info, a, uplo, diag, b, x, sweeps): an
    APPROXIMATE x = inv(A) b by Jacobi sweeps on the triangle triangular_solve reads (spblas_gfx950_sptrsv_sweeps; no reference
    counterpart).  x0_r = b_r / d_r, then `sweeps` times x_r = (b_r - sum of the row's strict entries times the PREVIOUS x) /
    d_r: one SpMV-shaped launch per sweep and no hand-off between levels -- what a preconditioner apply wants.  A row of level
    l is exact from sweep l on, so sweeps >= levels - 1 is the solve itself.  Operands as for triangular_solve with vectors
    (csr_view, float32 / float64, int32 offsets and columns, scaled(a), scaled(b)).  An info of triangular_solve_inspect for
    this matrix, triangle and diagonal narrows the later sweeps to the rows that can still change; without one every sweep
    covers all rows -- the call never inspects by itself.  The bits of x are the same either way.  A block of right-hand sides
    (2-D b / x) raises NotImplementedError."""
    info, (a, uplo, diag, b, x, sweeps) = _leading_info(args, 6, "a, uplo, diag, b, x, sweeps")
    bb = get_ultimate_base(b)
    if (_is_tensor(bb) and bb.dim() == 2) or (_is_tensor(x) and x.dim() == 2):
        raise NotImplementedError("gfx950 triangular_solve_sweeps: vectors only (a block of right-hand sides is not offered)")
    a_base = _trsv_operands(a, uplo, diag, b, x)
    if isinstance(sweeps, bool) or not isinstance(sweeps, int):
        raise TypeError("triangular_solve_sweeps: sweeps must be an int")
    if sweeps < 0 or sweeps > 2 ** 31 - 1:
        raise ValueError("triangular_solve_sweeps: sweeps must be a non-negative int")
    plan = info.state_ if info is not None and isinstance(info.state_, _TrsvPlan) else None
    if plan is not None and plan.key != _trsv_key(a_base, uplo, diag):
        plan = None  # another matrix, triangle or diagonal: plan-free (never a hidden inspect)
    hd = _Handle.current(a_base.rowptr().device)
    vt, ct = _vtype(a_base.values(), "triangular_solve_sweeps")
    sa = get_scaling_factor(a)
    alpha = ct(1 if sa is None else sa)
    sb = get_scaling_factor(b)
    if bb.numel() > 0 and bb.untyped_storage().data_ptr() == x.untyped_storage().data_ptr():
        bb = bb.clone()  # every sweep reads b while the iterates alternate between x and the work vector
    work = torch.empty_like(x) if sweeps > 0 else None
    check(_capi.lib().spblas_gfx950_sptrsv_sweeps(
        hd.h, plan.plan if plan is not None else None, a_base.shape()[0], a_base.size(), sweeps,
        _capi.UPPER if isinstance(uplo, upper_triangle_t) else _capi.LOWER,
        _capi.DIAG_UNIT if isinstance(diag, implicit_unit_diagonal_t) else _capi.DIAG_EXPLICIT, ctypes.byref(alpha),
        _ptr(a_base.rowptr()), _ptr(a_base.colind()), _ptr(a_base.values()), _ptr(bb), _ptr(x), _ptr(work), vt),
        "triangular_solve_sweeps")
    if sb is not None:  # the iteration is linear in b: sweeps(s b) = s sweeps(b)
        beta = ct(sb)
        check(_capi.lib().spblas_gfx950_scale(hd.h, x.numel(), ctypes.byref(beta), _ptr(x), vt), "triangular_solve_sweeps")


# --------------------------------------------------------------------------- ILU(0) (no reference counterpart)
class _Ilu0Plan(_NativePlan):
    """ilu0_inspect state: the lower level plan and the diagonal positions of A's pattern (spblas_gfx950_ilu0_create)."""
    _destroy, _info_call = "spblas_gfx950_ilu0_destroy", "spblas_gfx950_ilu0_info"
    _info_names = ("levels", "max_level_width", "launches_per_factor", "lanes_per_row")

    def status(self):
        row = ctypes.c_int64(-1)
        hd = _Handle.current(torch.device("cuda", self.hd.device))
        check(_capi.lib().spblas_gfx950_ilu0_status(hd.h, self.plan, ctypes.byref(row)), "spblas_gfx950_ilu0_status")
        return int(row.value)


def _square_csr_operand(a, what):
    """The square plain csr_view ilu0, multicolor_order, permute and gauss_seidel take; TypeError for every other operand, dtype
    or index type."""
    if not isinstance(a, csr_view):
        raise TypeError(f"{what}: the operand must be a plain csr_view (scaled, conjugated, transposed and csc_view "
                        f"operands are not supported), got {type(a).__name__}")
    vals = a.values()
    if not _is_tensor(vals) or not _is_tensor(a.rowptr()) or not _is_tensor(a.colind()):
        raise TypeError(f"{what}: values, row offsets and columns must be tensors")
    if vals.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: float32 / float64 values only, got {vals.dtype}")
    if a.rowptr().dtype != torch.int32 or a.colind().dtype != torch.int32:
        raise TypeError(f"{what}: int32 row offsets and columns only, got {a.rowptr().dtype} / {a.colind().dtype}")
    _check_csr(a, what)
    m, n = a.shape()
    if m != n:
        raise ValueError(f"{what}: matrix dimensions are incompatible (A must be square).")
    if a.rowptr().numel() < m + 1 or a.colind().numel() < a.size() or vals.numel() < a.size():
        raise ValueError(f"{what}: the arrays are shorter than the view's shape and size say")
    return a


def _structure_key(a):
    return (a.rowptr().data_ptr(), a.colind().data_ptr(), tuple(a.shape()), a.size())


def _perm_vector(perm, m, dev, what, optional=False):
    """perm as the inspects take it: a contiguous int32 vector of A's m rows on A's device (or None where it is optional)."""
    if perm is None and optional:
        return
    if not _is_tensor(perm) or perm.dtype != torch.int32:
        raise TypeError(f"{what}: perm must be an int32 tensor" + (" or None" if optional else ""))
    if perm.device != dev or not perm.is_contiguous() or perm.dim() != 1 or perm.numel() != m:
        raise ValueError(f"{what}: perm must be a contiguous vector of A's {m} rows on A's device")


def _ilu0_plan(a):
    hd = _Handle.current(a.rowptr().device)
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_ilu0_create(hd.h, ctypes.byref(plan), a.shape()[0], a.size(), _ptr(a.rowptr()),
                                               _ptr(a.colind()))
    if st == _capi.INVALID_VALUE:
        raise ValueError("ilu0_inspect: every row must hold strictly ascending columns inside [0, m) and its diagonal entry")
    check(st, "ilu0_inspect")
    return _Ilu0Plan(hd, plan, _structure_key(a), (a.rowptr(), a.colind()))


def ilu0_inspect(*args):
    """ilu0_inspect(a) -> operation_info_t, or ilu0_inspect(info, a): checks A's structure (sorted rows, stored diagonal;
    ValueError otherwise) and builds the level plan of the factorisation.  Synchronises the stream."""
    info, (a,) = _leading_info(args, 1, "a")
    ret = info is None
    if ret:
        info = operation_info_t()
    a = _square_csr_operand(a, "ilu0_inspect")
    info.state_ = _ilu0_plan(a)
    return info if ret else None


def _ilu0_lu_values(a, lu, what):
    """The value tensor of `lu`, a csr_view over A's own row offsets and columns."""
    if not isinstance(lu, csr_view):
        raise TypeError(f"{what}: lu must be a plain csr_view over A's structure, got {type(lu).__name__}")
    lv = lu.values()
    if not _is_tensor(lv) or lv.dtype != a.values().dtype:
        raise ValueError(f"{what}: lu's values must have A's value type {a.values().dtype}")
    if lv.device != a.values().device:
        raise ValueError(f"{what}: lu's values must live on A's device")
    if lv.numel() < a.size() or lu.size() != a.size() or tuple(lu.shape()) != tuple(a.shape()) or not lv.is_contiguous():
        raise ValueError(f"{what}: lu must have A's shape and a contiguous value array of at least A's number of entries")
    if lu.rowptr() is None or lu.colind() is None or lu.rowptr().data_ptr() != a.rowptr().data_ptr() or \
            lu.colind().data_ptr() != a.colind().data_ptr():
        raise ValueError(f"{what}: lu must be a view over A's own row offsets and columns")
    return lv


def _ilu0_plan_of(info, a):
    """The inspect result in `info` if it is this pattern's, else a new one (stored into `info`)."""
    plan = info.state_ if info is not None and isinstance(info.state_, _Ilu0Plan) else None
    if plan is None or plan.key != _structure_key(a):
        plan = _ilu0_plan(a)  # no usable inspect result: analyse now
        if info is not None:
            info.state_ = plan
    return plan


def ilu0(*args):
    """ilu0(a, lu) / ilu0(info, a, lu): the incomplete LU factorisation of A on A's own pattern, no pivoting (IKJ order, one fma
    per update: the same bits on every call).  `lu` is a csr_view over A's row offsets and columns with a value tensor of its own,
    or with A's value tensor (in place; `a` itself may be passed).  Its values hold L left of the diagonal (unit diagonal implied)
    and U on and right of it: the one view serves triangular_solve(lu, lower_triangle, implicit_unit_diagonal, b, y) and
    triangular_solve(lu, upper_triangle, explicit_diagonal, y, x).  Nothing is synchronised; ilu0_status(info) tells afterwards
    whether a pivot was zero or not finite."""
    info, (a, lu) = _leading_info(args, 2, "a, lu")
    a = _square_csr_operand(a, "ilu0")
    lv = _ilu0_lu_values(a, lu, "ilu0")
    plan = _ilu0_plan_of(info, a)
    hd = _Handle.current(a.rowptr().device)
    vt, _ = _vtype(a.values(), "ilu0")
    check(_capi.lib().spblas_gfx950_ilu0_factor(hd.h, plan.plan, a.shape()[0], a.size(), _ptr(a.rowptr()), _ptr(a.colind()),
                                                _ptr(a.values()), _ptr(lv), vt), "ilu0")
    _note_write(lv)


def ilu0_sweeps(*args):
    """ilu0_sweeps(a, lu, work, sweeps) / ilu0_sweeps(info, a, lu, work, sweeps): an APPROXIMATE ilu0 by fixed-point sweeps
    (spblas_gfx950_ilu0_sweeps; the row form of Chow and Patel's fine-grained ILU; no reference counterpart).  LU(0) = A, then
    `sweeps` times every row runs ilu0's elimination on A's row with the pivots and pivot rows of the PREVIOUS iterate: one
    launch per sweep and no hand-off between levels.  A row of level l has ilu0's bits from sweep l on, so sweeps >= levels - 1
    IS ilu0 (the count is clamped there).  Operands as for ilu0, but `lu` must own its values -- every sweep re-reads A, so there
    is no in-place form (ValueError).  `work` is a contiguous tensor of A's dtype and device with at least a.size() elements
    (unspecified afterwards), or None when sweeps <= 1.  Nothing is synchronised; ilu0_status(info) reports on the final
    pivots of the last sweep.  Without a usable inspect result the call analyses as ilu0 does."""
    info, (a, lu, work, sweeps) = _leading_info(args, 4, "a, lu, work, sweeps")
    a = _square_csr_operand(a, "ilu0_sweeps")
    lv = _ilu0_lu_values(a, lu, "ilu0_sweeps")
    if isinstance(sweeps, bool) or not isinstance(sweeps, int):
        raise TypeError("ilu0_sweeps: sweeps must be an int")
    if sweeps < 1 or sweeps > 2 ** 31 - 1:
        raise ValueError("ilu0_sweeps: sweeps must be a positive int")
    av = a.values()
    if a.size() > 0 and lv.data_ptr() == av.data_ptr():
        raise ValueError("ilu0_sweeps: lu must own its values (every sweep re-reads A: there is no in-place form)")
    if work is None:
        if sweeps > 1:
            raise ValueError("ilu0_sweeps: work may be None only when sweeps <= 1")
    else:
        if not _is_tensor(work):
            raise TypeError(f"ilu0_sweeps: work must be a tensor or None, got {type(work).__name__}")
        if work.dtype != av.dtype or work.device != av.device:
            raise ValueError(f"ilu0_sweeps: work must have A's value type {av.dtype} and live on A's device")
        if work.numel() < a.size() or not work.is_contiguous():
            raise ValueError("ilu0_sweeps: work must be contiguous and hold at least A's number of entries")
        if a.size() > 0 and work.data_ptr() in (av.data_ptr(), lv.data_ptr()):
            raise ValueError("ilu0_sweeps: work must be a buffer of its own, neither A's values nor lu's")
    plan = _ilu0_plan_of(info, a)
    hd = _Handle.current(a.rowptr().device)
    vt, _ = _vtype(av, "ilu0_sweeps")
    check(_capi.lib().spblas_gfx950_ilu0_sweeps(hd.h, plan.plan, a.shape()[0], a.size(), sweeps, _ptr(a.rowptr()),
                                                _ptr(a.colind()), _ptr(av), _ptr(lv), _ptr(work), vt), "ilu0_sweeps")
    _note_write(lv)
    if work is not None:
        _note_write(work)


def ilu0_status(info):
    """The smallest row whose pivot LU[i][i] was zero or not finite in the last ilu0 call on this inspect result, -1 if every
    pivot was finite and non-zero.  Synchronises the stream."""
    plan = getattr(info, "state_", None)
    if not isinstance(plan, _Ilu0Plan):
        raise TypeError("ilu0_status: expected the operation_info_t of ilu0_inspect / ilu0")
    return plan.status()


# ---- multicolour ordering and symmetric permutation (spblas_gfx950_multicolor_* / csr_permute_* / permute_vector) ----
class multicolor_order_t:
    """Result of multicolor_order: int32 device tensors `perm` (new -> old, sorted by (colour, old index)), `inverse`
    (old -> new), `color` (per row of A) and `color_ptr` (colours + 1 offsets into the new order), plus info()."""

    def __init__(self, perm, inverse, color, color_ptr, info):
        self.perm, self.inverse, self.color, self.color_ptr, self._info = perm, inverse, color, color_ptr, info

    def info(self):
        return dict(self._info)


def multicolor_order(a):
    """multicolor_order(a) -> multicolor_order_t: a deterministic distance-1 colouring of the graph of A + A^T (Jones-Plassmann
    with fixed priorities; the colours equal sequential greedy colouring in descending key order and depend on the pattern
    alone) and the permutation that sorts the rows by colour.  permute(a, order.perm, b) then gives a matrix whose two triangles
    have at most info()['colors'] levels for ilu0 / triangular_solve -- at the price of a weaker ILU(0) preconditioner than in
    the natural order.  `a` is a square plain csr_view (float32 / float64 values, int32 offsets and columns; rows need not be
    sorted, the pattern need not be symmetric).  Inspect-class: synchronises the stream, refused inside a capture."""
    a = _square_csr_operand(a, "multicolor_order")
    dev = a.rowptr().device
    hd = _Handle.current(dev)
    m = a.shape()[0]
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_multicolor_create(hd.h, ctypes.byref(plan), m, a.size(), _ptr(a.rowptr()), _ptr(a.colind()))
    if st == _capi.INVALID_VALUE:
        raise ValueError("multicolor_order: every column must lie inside [0, m) and the row offsets must describe the entries")
    check(st, "multicolor_order")
    try:
        arr = (ctypes.c_int64 * 4)()
        check(_capi.lib().spblas_gfx950_multicolor_info(plan, arr), "spblas_gfx950_multicolor_info")
        info = dict(zip(("colors", "rounds", "max_color_size", "lanes_per_row"), list(arr)))
        perm, inverse, color = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(3))
        color_ptr = torch.empty(info["colors"] + 1, dtype=torch.int32, device=dev)
        check(_capi.lib().spblas_gfx950_multicolor_copy(hd.h, plan, _ptr(perm), _ptr(inverse), _ptr(color), _ptr(color_ptr)),
              "spblas_gfx950_multicolor_copy")
    finally:
        _capi.lib().spblas_gfx950_multicolor_destroy(hd.h, plan)
    return multicolor_order_t(perm, inverse, color, color_ptr, info)


class _PermutePlan(_NativePlan):
    """permute_inspect state: the source position of every entry of B (spblas_gfx950_csr_permute_create)."""
    _destroy = "spblas_gfx950_csr_permute_destroy"


def _permute_operands(a, perm, b, what):
    a = _square_csr_operand(a, what)
    m, nnz = a.shape()[0], a.size()
    dev = a.rowptr().device
    _perm_vector(perm, m, dev, what)
    if not isinstance(b, csr_view):
        raise TypeError(f"{what}: b must be a plain csr_view over caller-allocated arrays, got {type(b).__name__}")
    bv, br, bc = b.values(), b.rowptr(), b.colind()
    if not _is_tensor(bv) or not _is_tensor(br) or not _is_tensor(bc):
        raise TypeError(f"{what}: b's values, row offsets and columns must be tensors")
    if br.dtype != torch.int32 or bc.dtype != torch.int32:
        raise TypeError(f"{what}: b must have int32 row offsets and columns, got {br.dtype} / {bc.dtype}")
    if bv.dtype != a.values().dtype:
        raise TypeError(f"{what}: b's values must have A's value type {a.values().dtype}, got {bv.dtype}")
    if any(t.device != dev or not t.is_contiguous() for t in (bv, br, bc)):
        raise ValueError(f"{what}: b's arrays must be contiguous and live on A's device")
    if tuple(b.shape()) != tuple(a.shape()):
        raise ValueError(f"{what}: matrix dimensions are incompatible (b must have A's shape).")
    if br.numel() < m + 1 or bc.numel() < nnz or bv.numel() < nnz:
        raise ValueError(f"{what}: b's arrays must hold {m + 1} row offsets and {nnz} columns and values")
    if br.data_ptr() == a.rowptr().data_ptr() or (nnz > 0 and (bc.data_ptr() == a.colind().data_ptr() or
                                                               bv.data_ptr() == a.values().data_ptr())):
        raise ValueError(f"{what}: b must have arrays of its own (there is no in-place form)")
    return a


def _permute_key(a, perm, b):
    return (a.rowptr().data_ptr(), a.colind().data_ptr(), tuple(a.shape()), a.size(), perm.data_ptr(),
            b.rowptr().data_ptr(), b.colind().data_ptr())


def _permute_plan(a, perm, b):
    hd = _Handle.current(a.rowptr().device)
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_csr_permute_create(hd.h, ctypes.byref(plan), a.shape()[0], a.size(), _ptr(a.rowptr()),
                                                      _ptr(a.colind()), _ptr(perm), _ptr(b.rowptr()), _ptr(b.colind()))
    if st == _capi.INVALID_VALUE:
        raise ValueError("permute_inspect: perm must be a permutation of 0 .. m - 1, every column of A must lie inside [0, m) "
                         "and A's row offsets must describe its entries")
    check(st, "permute_inspect")
    _note_write(b.colind())
    b.update(b.values(), b.rowptr(), b.colind(), a.shape(), a.size())
    return _PermutePlan(hd, plan, _permute_key(a, perm, b), (a.rowptr(), a.colind(), perm, b.rowptr(), b.colind()))


def permute_inspect(*args):
    """permute_inspect(a, perm, b) -> operation_info_t, or permute_inspect(info, a, perm, b): checks that `perm` (int32, new -> old)
    is a permutation (ValueError otherwise, with b untouched), writes the structure of B = P A P^T -- row i of B is row perm[i] of
    A with column c renamed to the new index of c, columns ascending, equal columns in source order -- into b's row offsets and
    columns, and keeps the source position of every entry.  `b` is a csr_view over caller-allocated arrays (m + 1 offsets, nnz
    columns and values) as for transpose.  Inspect-class: allocates, synchronises the stream, refused inside a capture."""
    info, (a, perm, b) = _leading_info(args, 3, "a, perm, b")
    ret = info is None
    if ret:
        info = operation_info_t()
    a = _permute_operands(a, perm, b, "permute_inspect")
    info.state_ = _permute_plan(a, perm, b)
    info.update_impl_(a.shape(), a.size())
    return info if ret else None


def permute(*args):
    """permute(a, perm, b) / permute(info, a, perm, b): B = P A P^T.  Without `info` the call inspects (permute_inspect) and fills
    b's values.  With the info of permute_inspect for these arrays it only gathers the values, b.values[p] = a.values[source of
    p]: one launch, nothing allocated or synchronised, so it can be recorded in a graph -- the refresh after A's values changed
    on a fixed pattern.  An info that was made for other arrays is replaced by a new inspect."""
    info, (a, perm, b) = _leading_info(args, 3, "a, perm, b")
    a = _permute_operands(a, perm, b, "permute")
    plan = info.state_ if info is not None and isinstance(info.state_, _PermutePlan) else None
    if plan is None or plan.key != _permute_key(a, perm, b):
        plan = _permute_plan(a, perm, b)  # no usable inspect result: analyse now
        if info is not None:
            info.state_ = plan
            info.update_impl_(a.shape(), a.size())
    hd = _Handle.current(a.rowptr().device)
    vt, _ = _vtype(a.values(), "permute")
    check(_capi.lib().spblas_gfx950_csr_permute_values(hd.h, plan.plan, a.size(), _ptr(a.values()), _ptr(b.values()), vt),
          "permute")
    _note_write(b.values())


def permute_vector(perm, src, dst, inverse=False):
    """permute_vector(perm, src, dst): dst[i] = src[perm[i]] -- b into the order of permute(a, perm, .); with inverse=True
    dst[perm[i]] = src[i] -- x back into A's order.  float32 / float64 vectors of perm's length, src and dst different buffers;
    perm is not checked here (permute_inspect does).  One launch, capturable."""
    if not _is_tensor(perm) or perm.dtype != torch.int32:
        raise TypeError("permute_vector: perm must be an int32 tensor")
    if not _is_tensor(src) or not _is_tensor(dst):
        raise TypeError("permute_vector: src and dst must be tensors")
    vt, _ = _vtype(src, "permute_vector")
    if dst.dtype != src.dtype:
        raise TypeError("permute_vector: src and dst must have one value type")
    n = perm.numel()
    if src.dim() != 1 or dst.dim() != 1 or perm.dim() != 1 or src.numel() != n or dst.numel() != n:
        raise ValueError("permute_vector: perm, src and dst must be vectors of one length")
    if not (perm.is_contiguous() and src.is_contiguous() and dst.is_contiguous()) or src.device != perm.device or \
            dst.device != perm.device:
        raise ValueError("permute_vector: the vectors must be contiguous and live on one device")
    if n > 0 and src.data_ptr() == dst.data_ptr():
        raise ValueError("permute_vector: src and dst must be different buffers")
    hd = _Handle.current(perm.device)
    check(_capi.lib().spblas_gfx950_permute_vector(hd.h, n, _ptr(perm), _ptr(src), _ptr(dst), vt, 1 if inverse else 0),
          "permute_vector")


# ---- multicolour Gauss-Seidel / SOR / SSOR sweeps (spblas_gfx950_gs_*; no reference counterpart) ----
class _GsPlan(_NativePlan):
    """gauss_seidel_inspect state: the colour offsets, the position of every row's diagonal entry and the row order
    (spblas_gfx950_gs_create).  Structure only, no values."""
    _destroy, _info_call = "spblas_gfx950_gs_destroy", "spblas_gfx950_gs_info"
    _info_names = ("colors", "max_color_size", "lanes_per_row", "launches_per_forward_sweep")


_GS_DIRECTIONS = {"forward": _capi.GS_FORWARD, "backward": _capi.GS_BACKWARD, "symmetric": _capi.GS_SYMMETRIC}


def gauss_seidel_inspect(*args, perm=None):
    """gauss_seidel_inspect(a, color_ptr, perm=None) -> operation_info_t, or gauss_seidel_inspect(info, a, color_ptr, perm=None):
    the inspect of gauss_seidel.  The row order is sigma(i) = perm[i] when a perm is given, else sigma(i) = i; colour c is the
    positions color_ptr[c] .. color_ptr[c + 1] - 1 of that order (multicolor_order's color_ptr: with order.perm on A itself,
    without a perm on the permuted B).  `a` is a square plain csr_view (float32 / float64 values, int32 offsets and columns);
    color_ptr and perm are contiguous int32 device vectors.  ValueError unless color_ptr starts at 0, is non-decreasing and ends
    at m (empty colours are allowed), perm is a permutation of 0 .. m - 1, the row offsets describe the entries, every column
    lies in [0, m), every row has exactly one stored diagonal entry and no stored off-diagonal entry joins two rows of one
    colour -- the last is what makes the in-place sweep race free, so it is checked and not assumed.  The result holds structure
    only (no values).  Inspect-class: allocates, synchronises the stream, refused inside a capture."""
    if len(args) >= 2 and isinstance(args[0], operation_info_t):
        info, ret, rest = args[0], False, args[1:]
    else:
        info, ret, rest = operation_info_t(), True, args
    if len(rest) == 3 and perm is None:
        a, color_ptr, perm = rest
    elif len(rest) == 2:
        a, color_ptr = rest
    else:
        raise TypeError("expected (a, color_ptr, perm=None) or (info, a, color_ptr, perm=None)")
    what = "gauss_seidel_inspect"
    a = _square_csr_operand(a, what)
    m = a.shape()[0]
    dev = a.rowptr().device
    if not _is_tensor(color_ptr) or color_ptr.dtype != torch.int32:
        raise TypeError(f"{what}: color_ptr must be an int32 tensor")
    if color_ptr.device != dev or not color_ptr.is_contiguous() or color_ptr.dim() != 1 or color_ptr.numel() < 1:
        raise ValueError(f"{what}: color_ptr must be a contiguous vector of colours + 1 offsets on A's device")
    _perm_vector(perm, m, dev, what, optional=True)
    hd = _Handle.current(dev)
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_gs_create(hd.h, ctypes.byref(plan), m, a.size(), _ptr(a.rowptr()), _ptr(a.colind()),
                                             color_ptr.numel() - 1, _ptr(color_ptr), _ptr(perm))
    if st == _capi.INVALID_VALUE:
        raise ValueError(f"{what}: color_ptr must run from 0 to m without descending, perm must be a permutation of 0 .. m - 1, "
                         "the row offsets must describe the entries with every column inside [0, m), every row must store "
                         "exactly one diagonal entry and no off-diagonal entry may join two rows of one colour")
    check(st, what)
    info.state_ = _GsPlan(hd, plan, _structure_key(a), (a.rowptr(), a.colind()))
    info.update_impl_(a.shape(), a.size())
    return info if ret else None


def gauss_seidel(info, a, b, x, sweeps=1, omega=1.0, direction="forward"):
    """gauss_seidel(info, a, b, x, sweeps=1, omega=1.0, direction="forward"): multicolour Gauss-Seidel / SOR sweeps on A x = b,
    x updated IN PLACE (spblas_gfx950_gs_sweep; no reference counterpart).  The colouring lives in `info`, the result of
    gauss_seidel_inspect for these row offsets and columns (anything else: ValueError -- the call never inspects by itself).
    One row update is  dot = sum of a_rc x_c over the stored entries with c != r;  g = (b_r - dot) / d_r;  x_r = g when
    omega == 1 (the old x_r is not read), else x_r = fma(omega, g - x_r, x_r).  "forward" updates the colours 0 .. C - 1 one after
    the other, "backward" C - 1 .. 0, "symmetric" forward then backward; `sweeps` repeats that (0: x untouched, nothing
    launched).  One symmetric sweep from x = 0 is the SSOR preconditioner.  The result equals sequential Gauss-Seidel in colour
    order bit for bit and does not depend on the grid, earlier calls or graph capture.  A's values are read as they are at the
    call (the info holds structure only); b is only read.  One launch per non-empty colour and half-sweep, nothing allocated or
    synchronised: recordable in a graph from the first call.  `a`: square plain csr_view, float32 / float64, int32 indices; b and
    x: contiguous vectors of m elements of A's type on A's device in different buffers (scaled(b) is refused); omega is taken as
    given.  Not offered: a block of right-hand sides, weighted Jacobi, an implied zero initial guess, several colours per
    launch, scaled / complex / 16-bit / int64 / csc_view operands, distance-2 colourings."""
    what = "gauss_seidel"
    a = _square_csr_operand(a, what)
    m = a.shape()[0]
    av = a.values()
    for name, t in (("b", b), ("x", x)):
        if not _is_tensor(t):
            raise TypeError(f"{what}: {name} must be a tensor (scaled and other views are not supported), got {type(t).__name__}")
        if t.dtype != av.dtype:
            raise TypeError(f"{what}: {name} must have A's value type {av.dtype}, got {t.dtype}")
        if t.dim() == 2:
            raise NotImplementedError(f"{what}: vectors only (a block of right-hand sides is not offered)")
        if t.dim() != 1 or t.numel() != m or not t.is_contiguous() or t.device != av.device:
            raise ValueError(f"{what}: {name} must be a contiguous vector of A's {m} rows on A's device")
    if m > 0 and b.data_ptr() == x.data_ptr():
        raise ValueError(f"{what}: b and x must be different buffers")
    if isinstance(sweeps, bool) or not isinstance(sweeps, int):
        raise TypeError(f"{what}: sweeps must be an int")
    if sweeps < 0 or sweeps > 2 ** 31 - 1:
        raise ValueError(f"{what}: sweeps must be a non-negative int")
    if isinstance(omega, bool) or not isinstance(omega, (int, float)):
        raise TypeError(f"{what}: omega must be a real number")
    if not isinstance(direction, str) or direction not in _GS_DIRECTIONS:
        raise ValueError(f"{what}: direction must be 'forward', 'backward' or 'symmetric'")
    plan = getattr(info, "state_", None)
    if not isinstance(plan, _GsPlan) or plan.key != _structure_key(a):
        raise ValueError(f"{what}: info must be the result of gauss_seidel_inspect for these row offsets and columns")
    hd = _Handle.current(a.rowptr().device)
    vt, ct = _vtype(av, what)
    w = ct(omega)
    check(_capi.lib().spblas_gfx950_gs_sweep(hd.h, plan.plan, m, a.size(), sweeps, _GS_DIRECTIONS[direction], ctypes.byref(w),
                                             _ptr(a.rowptr()), _ptr(a.colind()), _ptr(av), _ptr(b), _ptr(x), vt), what)
    if sweeps > 0:
        _note_write(x)


# ---- MIS-2 aggregation and the Galerkin coarse matrix (spblas_gfx950_aggregate_* / coarsen_*; no reference counterpart) ----
class _AggregatePlan(_NativePlan):
    """aggregate state: agg and root on the device, what prolongator() reads (spblas_gfx950_aggregate_create)."""
    _destroy = "spblas_gfx950_aggregate_destroy"


def _csr_target(c, shape, nnz, dtype, dev, what, name):
    """A caller-allocated plain csr_view the call writes into: int32 offsets and columns, values of `dtype`, long enough."""
    if not isinstance(c, csr_view):
        raise TypeError(f"{what}: {name} must be a plain csr_view over caller-allocated arrays, got {type(c).__name__}")
    cv, cr, cc = c.values(), c.rowptr(), c.colind()
    if not _is_tensor(cv) or not _is_tensor(cr) or not _is_tensor(cc):
        raise TypeError(f"{what}: {name}'s values, row offsets and columns must be tensors")
    if cr.dtype != torch.int32 or cc.dtype != torch.int32:
        raise TypeError(f"{what}: {name} must have int32 row offsets and columns, got {cr.dtype} / {cc.dtype}")
    if cv.dtype != dtype:
        raise TypeError(f"{what}: {name}'s values must have the value type {dtype}, got {cv.dtype}")
    if any(t.device != dev or not t.is_contiguous() for t in (cv, cr, cc)):
        raise ValueError(f"{what}: {name}'s arrays must be contiguous and live on the operand's device")
    if cr.numel() < shape[0] + 1 or cc.numel() < nnz or cv.numel() < nnz:
        raise ValueError(f"{what}: {name}'s arrays must hold {shape[0] + 1} row offsets and {nnz} columns and values")
    return c


class aggregate_t:
    """Result of aggregate: int32 device tensors `agg` (the aggregate of every row) and `root` (the root row of every
    aggregate, ascending), `n_agg`, info() and prolongator()."""

    def __init__(self, agg, root, n_agg, info, plan, m):
        self.agg, self.root, self.n_agg, self._info, self._plan, self._m = agg, root, n_agg, info, plan, m

    def info(self):
        return dict(self._info)

    def prolongator(self, p):
        """prolongator(dtype) -> csr_view, or prolongator(p): the tentative prolongator P, m x n_agg, row offsets 0 .. m, columns
        `agg`, values 1 (float32 / float64).  With a caller-allocated csr_view `p` (m + 1 offsets, m columns and values) it is
        one launch, nothing allocated or synchronised: recordable in a graph."""
        what = "prolongator"
        m, dev = self._m, self.agg.device
        if isinstance(p, torch.dtype):
            if p not in (torch.float32, torch.float64):
                raise TypeError(f"{what}: float32 / float64 values only, got {p}")
            p = csr_view(torch.empty(m, dtype=p, device=dev), torch.empty(m + 1, dtype=torch.int32, device=dev),
                         torch.empty(m, dtype=torch.int32, device=dev), (m, self.n_agg), m)
            ret = True
        else:
            ret = False
            if isinstance(p, csr_view) and _is_tensor(p.values()) and p.values().dtype not in (torch.float32, torch.float64):
                raise TypeError(f"{what}: float32 / float64 values only, got {p.values().dtype}")
            _csr_target(p, (m, self.n_agg), m, p.values().dtype if isinstance(p, csr_view) and _is_tensor(p.values()) else None,
                        dev, what, "p")
        hd = _Handle.current(dev)
        vt, _ = _vtype(p.values(), what)
        check(_capi.lib().spblas_gfx950_aggregate_prolongator(hd.h, self._plan.plan, m, _ptr(p.rowptr()), _ptr(p.colind()),
                                                              _ptr(p.values()), vt), what)
        _note_write(p.values(), p.colind())
        p.update(p.values(), p.rowptr(), p.colind(), (m, self.n_agg), m)
        return p if ret else None


def aggregate(a, theta=0.0):
    """aggregate(a, theta=0.0) -> aggregate_t: groups the rows of A into aggregates around the roots of a maximal independent set
    at distance 2 of the strength graph (MIS-2 aggregation after Bell, Dalton and Olson; no reference counterpart).  In A's value
    type T, with d_i the first stored diagonal entry of row i (0 without one) and t2 = T(theta * theta), a stored off-diagonal
    a_ij is strong iff a_ij * a_ij >= (t2 * |d_i|) * |d_j|; a NaN on either side makes it weak; theta = 0 keeps every stored
    off-diagonal entry.  Rows i and j are neighbours iff a_ij or a_ji is strong.  The roots are greedy MIS on the square of that
    graph in descending order of the fixed keys multicolor_order uses: they, the aggregates and the number of rounds depend on
    the pattern, the values and theta alone.  A row without a strong neighbour is an aggregate of its own.  `a` is a square plain
    csr_view (float32 / float64 values, int32 offsets and columns; rows need not be sorted, the pattern need not be symmetric).
    Inspect-class: synchronises the stream, refused inside a capture."""
    what = "aggregate"
    a = _square_csr_operand(a, what)
    if isinstance(theta, bool) or not isinstance(theta, (int, float)):
        raise TypeError(f"{what}: theta must be a real number")
    theta = float(theta)
    if not (theta >= 0.0) or theta == float("inf"):
        raise ValueError(f"{what}: theta must be finite and >= 0")
    dev = a.rowptr().device
    hd = _Handle.current(dev)
    m = a.shape()[0]
    vt, _ = _vtype(a.values(), what)
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_aggregate_create(hd.h, ctypes.byref(plan), m, a.size(), _ptr(a.rowptr()), _ptr(a.colind()),
                                                    _ptr(a.values()), ctypes.c_double(theta), vt)
    if st == _capi.INVALID_VALUE:
        raise ValueError(f"{what}: every column must lie inside [0, m) and the row offsets must describe the entries")
    check(st, what)
    owner = _AggregatePlan(hd, plan, None)
    arr = (ctypes.c_int64 * 8)()
    check(_capi.lib().spblas_gfx950_aggregate_info(plan, arr), "spblas_gfx950_aggregate_info")
    info = dict(zip(("aggregates", "rounds", "largest", "smallest", "singletons", "strong_entries", "lanes_per_row"), list(arr)))
    n_agg = info["aggregates"]
    agg = torch.empty(m, dtype=torch.int32, device=dev)
    root = torch.empty(n_agg, dtype=torch.int32, device=dev)
    check(_capi.lib().spblas_gfx950_aggregate_copy(hd.h, plan, _ptr(agg), _ptr(root)), "spblas_gfx950_aggregate_copy")
    return aggregate_t(agg, root, n_agg, info, owner, m)


class _CoarsenPlan(_NativePlan):
    """coarsen_inspect state: the structure of A_c, the first sorted position of every coarse entry and the source position of
    every sorted position (spblas_gfx950_coarsen_create)."""
    _destroy, _info_call = "spblas_gfx950_coarsen_destroy", "spblas_gfx950_coarsen_info"
    _info_names = ("n_agg", "nnz", "fine_rows", "fine_nnz")


def _coarsen_operands(a, agg, n_agg, what):
    a = _square_csr_operand(a, what)
    m = a.shape()[0]
    if not _is_tensor(agg) or agg.dtype != torch.int32:
        raise TypeError(f"{what}: agg must be an int32 tensor")
    if agg.device != a.rowptr().device or not agg.is_contiguous() or agg.dim() != 1 or agg.numel() != m:
        raise ValueError(f"{what}: agg must be a contiguous vector of A's {m} rows on A's device")
    if isinstance(n_agg, bool) or not isinstance(n_agg, int):
        raise TypeError(f"{what}: n_agg must be an int")
    if n_agg < 0 or n_agg >= 2 ** 31 - 1:
        raise ValueError(f"{what}: n_agg must be a non-negative int32")
    return a


def _coarsen_key(a, agg, n_agg):
    return (a.rowptr().data_ptr(), a.colind().data_ptr(), tuple(a.shape()), a.size(), agg.data_ptr(), n_agg)


def _coarsen_plan(a, agg, n_agg):
    hd = _Handle.current(a.rowptr().device)
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_coarsen_create(hd.h, ctypes.byref(plan), a.shape()[0], a.size(), _ptr(a.rowptr()),
                                                  _ptr(a.colind()), _ptr(agg), n_agg)
    if st == _capi.INVALID_VALUE:
        raise ValueError("coarsen_inspect: every entry of agg must lie inside [0, n_agg), every column of A inside [0, m) and "
                         "A's row offsets must describe its entries")
    check(st, "coarsen_inspect")
    return _CoarsenPlan(hd, plan, _coarsen_key(a, agg, n_agg), (a.rowptr(), a.colind(), agg))


def _coarsen_set(info, plan):
    info.state_ = plan
    pi = plan.info()
    info.update_impl_((pi["n_agg"], pi["n_agg"]), pi["nnz"])
    info.shape, info.nnz = (pi["n_agg"], pi["n_agg"]), pi["nnz"]


def coarsen_inspect(*args):
    """coarsen_inspect(a, agg, n_agg) -> operation_info_t, or coarsen_inspect(info, a, agg, n_agg): the structure of the Galerkin
    coarse matrix A_c = P^T A P for the piecewise-constant P of ANY int32 map `agg` (m entries in [0, n_agg); ValueError
    otherwise) -- A need not have been aggregated by aggregate().  Entry p of A becomes (agg[row], agg[col]); equal pairs collapse
    to one entry of A_c; an aggregate without rows gives an empty row.  info.shape and info.nnz (also result_shape() /
    result_nnz()) say what to allocate for A_c.  Inspect-class: allocates, synchronises the stream, refused inside a capture."""
    info, (a, agg, n_agg) = _leading_info(args, 3, "a, agg, n_agg")
    ret = info is None
    if ret:
        info = operation_info_t()
    a = _coarsen_operands(a, agg, n_agg, "coarsen_inspect")
    _coarsen_set(info, _coarsen_plan(a, agg, n_agg))
    return info if ret else None


def _coarsen_info_plan(info, what):
    plan = getattr(info, "state_", None)
    if not isinstance(plan, _CoarsenPlan):
        raise TypeError(f"{what}: expected the operation_info_t of coarsen_inspect")
    return plan


def coarsen_structure(info, a_c):
    """coarsen_structure(info, a_c): writes A_c's row offsets and its ascending, duplicate-free columns into the caller-allocated
    csr_view `a_c` (info.shape[0] + 1 offsets, info.nnz columns and values).  Copies on the stream: recordable."""
    what = "coarsen_structure"
    plan = _coarsen_info_plan(info, what)
    pi = plan.info()
    n, cn = pi["n_agg"], pi["nnz"]
    dev = plan.tensors[0].device
    if isinstance(a_c, csr_view) and _is_tensor(a_c.values()):
        _vtype(a_c.values(), what)
    _csr_target(a_c, (n, n), cn, a_c.values().dtype if isinstance(a_c, csr_view) and _is_tensor(a_c.values()) else None, dev,
                what, "a_c")
    hd = _Handle.current(dev)
    check(_capi.lib().spblas_gfx950_coarsen_structure(hd.h, plan.plan, _ptr(a_c.rowptr()), _ptr(a_c.colind())), what)
    _note_write(a_c.colind())
    a_c.update(a_c.values(), a_c.rowptr(), a_c.colind(), (n, n), cn)


def _overlap(s, t):
    """True iff two tensors share bytes."""
    if s.numel() == 0 or t.numel() == 0 or s.untyped_storage().data_ptr() != t.untyped_storage().data_ptr():
        return False
    s0, t0 = s.data_ptr(), t.data_ptr()
    return s0 < t0 + t.numel() * t.element_size() and t0 < s0 + s.numel() * s.element_size()


def coarsen(info, a, a_c):
    """coarsen(info, a, a_c): the VALUES of A_c = P^T A P: a_c.values[e] = the sum of the values of A's entries that were renamed
    to coarse entry e, added one after the other in ascending source position, plain additions in A's value type from the first
    term -- the bits depend on A and agg alone.  One launch, nothing allocated or synchronised: recordable in a graph from its
    first use, the refresh after A's values changed on a fixed pattern.  `info` is the result of coarsen_inspect; when it was made
    for other row offset / column arrays than a's, it is replaced by a new inspect of `a` with the same agg and n_agg (which is
    inspect-class).  a_c's structure is written by coarsen_structure; only its first info.nnz values are written here.  a_c must
    not alias A's arrays.
    Not offered: a restriction other than P^T, weights in P (smooth_prolongator makes the smoothed P; A_c for it is two
    SpGEMMs), scaled / complex / 16-bit / int64 operands."""
    what = "coarsen"
    plan = _coarsen_info_plan(info, what)
    agg, n_agg = plan.tensors[2], plan.key[-1]
    a = _coarsen_operands(a, agg, n_agg, what)
    if plan.key != _coarsen_key(a, agg, n_agg):
        plan = _coarsen_plan(a, agg, n_agg)  # made for other arrays: analyse now
        _coarsen_set(info, plan)
    pi = plan.info()
    n, cn = pi["n_agg"], pi["nnz"]
    av = a.values()
    _csr_target(a_c, (n, n), cn, av.dtype, av.device, what, "a_c")
    cv = a_c.values()
    if any(_overlap(x, y) for x in (cv, a_c.rowptr(), a_c.colind()) for y in (av, a.rowptr(), a.colind(), agg)):
        raise ValueError(f"{what}: a_c must have arrays of its own (there is no in-place form)")
    hd = _Handle.current(av.device)
    vt, _ = _vtype(av, what)
    check(_capi.lib().spblas_gfx950_coarsen_values(hd.h, plan.plan, a.size(), _ptr(av), cn, _ptr(cv), vt), what)
    _note_write(cv)


# ---- the smoothed prolongator of smoothed aggregation (spblas_gfx950_smooth_*; no reference counterpart) ----
class _SmoothPlan(_NativePlan):
    """smooth_prolongator_inspect state: the structure of P, the first sorted position of every entry of P, the source position
    of every sorted position and the work array of the value pass (spblas_gfx950_smooth_create)."""
    _destroy, _info_call = "spblas_gfx950_smooth_destroy", "spblas_gfx950_smooth_info"
    _info_names = ("n_agg", "nnz", "fine_rows", "fine_nnz")


def _smooth_plan(a, agg, n_agg):
    hd = _Handle.current(a.rowptr().device)
    plan = ctypes.c_void_p()
    st = _capi.lib().spblas_gfx950_smooth_create(hd.h, ctypes.byref(plan), a.shape()[0], a.size(), _ptr(a.rowptr()),
                                                 _ptr(a.colind()), _ptr(agg), n_agg)
    if st == _capi.INVALID_VALUE:
        raise ValueError("smooth_prolongator_inspect: every entry of agg must lie inside [0, n_agg), every column of A inside "
                         "[0, m) and A's row offsets must describe its entries")
    check(st, "smooth_prolongator_inspect")
    return _SmoothPlan(hd, plan, _coarsen_key(a, agg, n_agg), (a.rowptr(), a.colind(), agg))


def _smooth_set(info, plan):
    info.state_ = plan
    pi = plan.info()
    info.update_impl_((pi["fine_rows"], pi["n_agg"]), pi["nnz"])
    info.shape, info.nnz = (pi["fine_rows"], pi["n_agg"]), pi["nnz"]


def smooth_prolongator_inspect(*args):
    """smooth_prolongator_inspect(a, agg, n_agg) -> operation_info_t, or smooth_prolongator_inspect(info, a, agg, n_agg): the
    structure of the smoothed prolongator P = (I - omega D_F^-1 A_F) T for the piecewise-constant T of ANY int32 map `agg` (m
    entries in [0, n_agg); ValueError otherwise).  Row i of P holds one entry for every distinct aggregate among agg[i] and the
    agg[j] of row i's stored entries, columns ascending -- whatever the values are: a weak or cancelling contribution leaves an
    explicit zero.  info.shape = (m, n_agg) and info.nnz (also result_shape() / result_nnz()) say what to allocate for P.
    Value-free.  Inspect-class: allocates, synchronises the stream, refused inside a capture.  One info serves one stream at a
    time (it holds a work array the value pass rewrites)."""
    info, (a, agg, n_agg) = _leading_info(args, 3, "a, agg, n_agg")
    ret = info is None
    if ret:
        info = operation_info_t()
    a = _coarsen_operands(a, agg, n_agg, "smooth_prolongator_inspect")
    _smooth_set(info, _smooth_plan(a, agg, n_agg))
    return info if ret else None


def _smooth_info_plan(info, what):
    plan = getattr(info, "state_", None)
    if not isinstance(plan, _SmoothPlan):
        raise TypeError(f"{what}: expected the operation_info_t of smooth_prolongator_inspect")
    return plan


def smooth_prolongator_structure(info, p):
    """smooth_prolongator_structure(info, p): writes P's row offsets and its ascending, duplicate-free columns into the
    caller-allocated csr_view `p` (info.shape[0] + 1 offsets, info.nnz columns and values).  Copies on the stream: recordable."""
    what = "smooth_prolongator_structure"
    plan = _smooth_info_plan(info, what)
    pi = plan.info()
    shape, pn = (pi["fine_rows"], pi["n_agg"]), pi["nnz"]
    dev = plan.tensors[0].device
    if isinstance(p, csr_view) and _is_tensor(p.values()):
        _vtype(p.values(), what)
    _csr_target(p, shape, pn, p.values().dtype if isinstance(p, csr_view) and _is_tensor(p.values()) else None, dev, what, "p")
    hd = _Handle.current(dev)
    check(_capi.lib().spblas_gfx950_smooth_structure(hd.h, plan.plan, _ptr(p.rowptr()), _ptr(p.colind())), what)
    _note_write(p.colind())
    p.update(p.values(), p.rowptr(), p.colind(), shape, pn)


def smooth_prolongator(info, a, p, omega, theta=0.0):
    """smooth_prolongator(info, a, p, omega, theta=0.0): the VALUES of P = (I - omega D_F^-1 A_F) T, fixed to the bit in A's value
    type T.  With the strength rule of aggregate (d_i the first stored diagonal entry, t2 = T(theta * theta), a_ij strong iff
    j != i and a_ij * a_ij >= (t2 * |d_i|) * |d_j|):  dF_i = T(0) plus, in ascending stored position, every entry of row i on
    the diagonal (repeats included) or weak;  when dF_i is finite and non-zero, s_i = T(omega) / dF_i and base_i = T(1) -
    T(omega), else s_i = 0 and base_i = 1 (the row of T);  P(i, J) = fma(-s_i, acc, b) with acc = T(0) plus the strong entries
    of row i whose column lies in aggregate J, in ascending position, and b = base_i if J == agg[i] else 0.  theta = 0 makes
    every finite off-diagonal entry strong; omega = 0 gives T on P's pattern.  The bits depend on A, agg, omega and theta alone.
    Two launches, nothing allocated or synchronised: recordable in a graph from its first use, the refresh after A's values
    changed on a fixed pattern.  `info` is the result of smooth_prolongator_inspect; when it was made for other row offset /
    column arrays than a's, it is replaced by a new inspect of `a` with the same agg and n_agg (which is inspect-class).  p's
    structure is written by smooth_prolongator_structure; only its first info.nnz values are written here.  p must not alias
    A's arrays.  omega must be finite, theta finite and >= 0.
    Not offered: an estimate of the spectral radius of D^-1 A (the caller supplies omega), a hierarchy or cycle driver, a fused
    P^T A P for this P (transpose and two multiply calls do it), scaled / complex / 16-bit / int64 / CSC operands."""
    what = "smooth_prolongator"
    plan = _smooth_info_plan(info, what)
    agg, n_agg = plan.tensors[2], plan.key[-1]
    a = _coarsen_operands(a, agg, n_agg, what)
    for name, x in (("omega", omega), ("theta", theta)):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise TypeError(f"{what}: {name} must be a real number")
    omega, theta = float(omega), float(theta)
    if omega != omega or omega in (float("inf"), float("-inf")):
        raise ValueError(f"{what}: omega must be finite")
    if not (theta >= 0.0) or theta == float("inf"):
        raise ValueError(f"{what}: theta must be finite and >= 0")
    if plan.key != _coarsen_key(a, agg, n_agg):
        plan = _smooth_plan(a, agg, n_agg)  # made for other arrays: analyse now
        _smooth_set(info, plan)
    pi = plan.info()
    shape, pn = (pi["fine_rows"], pi["n_agg"]), pi["nnz"]
    av = a.values()
    _csr_target(p, shape, pn, av.dtype, av.device, what, "p")
    pv = p.values()
    if any(_overlap(x, y) for x in (pv, p.rowptr(), p.colind()) for y in (av, a.rowptr(), a.colind(), agg)):
        raise ValueError(f"{what}: p must have arrays of its own (there is no in-place form)")
    hd = _Handle.current(av.device)
    vt, ctype = _vtype(av, what)
    w = ctype(omega)
    if not np.isfinite(w.value):
        raise ValueError(f"{what}: omega must be finite in A's value type")
    check(_capi.lib().spblas_gfx950_smooth_values(hd.h, plan.plan, a.shape()[0], a.size(), _ptr(a.rowptr()), _ptr(a.colind()),
                                                  _ptr(av), ctypes.byref(w), ctypes.c_double(theta), pn, _ptr(pv), vt), what)
    _note_write(pv)
