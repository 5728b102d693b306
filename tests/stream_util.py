"""Cases and helpers of the stream-order tests (tests/test_gpu_stream_order.py runs them on the device,
tests/test_stream_order_cpu.py proves the generators on the host).

THE CONTRACT UNDER TEST.  Every entry point takes its order from one place: the stream the handle is bound to at the call (the
Python layer binds it to torch's current stream).  Nothing a call issues -- a memset, a copy, a count read-back, a helper
kernel -- may run on the null stream or on a stream the handle sat on earlier.

HOW A CASE SHOWS IT.  A case is one op form.  Its device buffers hold DECOY inputs; on a side stream a filler kernel (hold)
keeps the stream busy for about 30 ms, behind it the REAL inputs are copied over the decoys in stream order, then the op is
called.  Whatever the op launched out of stream order runs while the hold is still in force, reads decoys (or writes an output
the later in-order kernels overwrite only in part) and the result misses expected(real).  Index arrays are never written late:
both input sets live on one structure, so a misordered read gives wrong numbers, never an access out of range.

DATA.  No tolerance is introduced here.  Every value family is exact: small integers or dyadic fractions on which every
product, every partial sum in any order and every division is exact in the value type, so the device must return the float64
host result BIT FOR BIT (sweeps_util.bit_violations / ilu_util.exact_violations / ladder.bits_equal, as the op's own test file
does on its exact families), and a decoy result differs from the real one in EVERY output element (host-checked: separated()).
Expected values come from the helpers the op's own tests use: oracle.spmv / spmm / spgemm_numeric(_d) / add / transpose,
scipy in complex128 for the complex paths (tests/test_gpu_complex.py), ladder_tt.trsv_system (x_true), sweeps_util.reference,
ilu_util.split_lu on the exact family of ilu_util.exact_system, gs_util.reference, multicolor_util.model_colors / host_permute.

CLASSES.  A call that only launches is execute-class: the test asserts that the side stream is still busy right after the
enqueue AND that the event recorded behind the hold has not fired (after a wait inside a call the stream is busy again with the
call's own last kernels, so the stream alone would not tell).  A call that synchronises, reads a count back, may free memory
(hipFree waits for the device) or is refused inside a capture is inspect-class in the variants named by Case.sync, with the
reason in Case.why: there the test asserts instead that the hold was at least ten times as long as the host took from
enqueueing it to entering the call -- everything such a call issues before its first wait is then issued under the hold.
"""
import contextlib
import functools
import os
import types

import numpy as np
import scipy.sparse as sps
import torch

import gs_util as GS
import ilu_util as IU
import ladder
import ladder_tt as TT
import multicolor_util as MC
import spblas_reference_amd as sp
import sweeps_util as SW
from oracle import oracle
from spblas_reference_amd import _capi
from spblas_reference_amd.api import _Handle

HOLD_MS = 30.0
VARIANTS = ("fresh", "warmed")
LOWP = (torch.float16, torch.bfloat16)


# ====================================================================================================================== hold
_CYCLES_PER_MS = None


def _timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _filler(units):
    """One unit of busy time on the current stream: torch's spin kernel, or (a torch without it) a chain of small matmuls."""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
        return
    if not hasattr(_filler, "eye"):
        _filler.eye = torch.eye(512, device="cuda")
    a = _filler.eye
    for _ in range(max(1, int(units) // 100_000)):       # (calibrate() scales `units` to this chain as it does to the spin)
        a = a @ _filler.eye


def calibrate():
    """Scales the filler once per process from one event-timed call on the current stream (synchronises the device):
    calibration, not an assertion -- the tests measure the hold they got."""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        probe = 4_000_000
        _filler(probe)                                   # (first call: loads the kernel)
        _CYCLES_PER_MS = probe / max(_timed_ms(lambda: _filler(probe)), 1e-3)
    return _CYCLES_PER_MS


def hold(stream, ms=HOLD_MS):
    """Enqueues a filler that keeps `stream` busy for about `ms` milliseconds."""
    per_ms = calibrate()
    with torch.cuda.stream(stream):
        _filler(ms * per_ms)


def device_form(case, arrays):
    """Host arrays as the device would return them: rounded once to the case's value type (index arrays as they are)."""
    out = []
    for a in arrays:
        a = np.asarray(a)
        if a.dtype.kind in "iu":
            out.append(a)
        elif case.dtype in LOWP:
            out.append(torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(case.dtype))
        else:
            out.append(a.astype({torch.float32: np.float32, torch.float64: np.float64,
                                 torch.complex64: np.complex64}[case.dtype]))
    return out


# ================================================================================================================== helpers
def to_dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to("cuda")
    return t if dtype is None else t.to(dtype)


def to_host(t):
    """numpy for the types numpy has, a host tensor for the 16-bit ones."""
    t = t.detach().cpu()
    return t if t.dtype in LOWP else t.numpy()


def prefill(t):
    """What an output holds before the op: NaN (values), -1 (indices)."""
    if t.is_complex():
        t.fill_(complex(float("nan"), float("nan")))
    elif t.is_floating_point():
        t.fill_(float("nan"))
    else:
        t.fill_(-1)


def _flat(a):
    if isinstance(a, torch.Tensor):
        return a.float().numpy().ravel()
    return np.asarray(a).ravel()


def bit_violations(got, want, what=""):
    """Messages (empty: passes): one output against its float64 / complex128 / integer expectation, bit for bit.  Floats go
    through sweeps_util.bit_violations (the comparison of the exact dyadic families), 16-bit tensors through ladder.bits_equal,
    index arrays through array_equal."""
    if isinstance(got, torch.Tensor):
        ok = tuple(got.shape) == tuple(np.shape(want)) and ladder.bits_equal(got, np.asarray(want, np.float64), got.dtype)
        return [] if ok else [f"{what}: the {got.dtype} output differs from the rounded float64 result"]
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind in "iu":
        return [] if got.shape == want.shape and np.array_equal(got, want) else \
            [f"{what}: index arrays differ ({int((got != want).sum()) if got.shape == want.shape else 'shapes'})"]
    if got.dtype.kind == "c":
        real = np.float32 if got.dtype == np.complex64 else np.float64
        want = np.ascontiguousarray(want.astype(got.dtype)).view(real)
        got = np.ascontiguousarray(got).view(real)
    return SW.bit_violations(got, want, what)


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ================================================================================================================ host data
M_ROWS, N_COLS = 3000, 2500            # the SpMV / SpMM / transpose operand: 6 ... 24 entries per row, every column used
NB = (3, 64)                           # the column counts of the dense operands


def exact_pattern(m, n, lo, hi, seed):
    """(rowptr, colind) int32: lo ... hi distinct ascending columns per row, column r mod n among those of row r (so with
    m >= n every column holds an entry: no output element of the transposed product is an empty sum)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, m)
    rows = []
    for r in range(m):
        c = set(int(v) for v in rng.choice(n, int(lens[r]) - 1, replace=False))
        c.add(r % n)
        rows.append(sorted(c))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


@functools.lru_cache(maxsize=None)
def operand():
    """The shared sparse operand and its dense partners, all positive small integers: a row holds at most 24 entries of at most
    2, x and B at most 3, so every sum is an integer below 256 -- exact in bfloat16, float16, float32 in any order; a column
    holds fewer than 100 entries (asserted), which keeps the transposed sums exact in float32.  The decoys: values times 3, the
    dense operand negated -- the result is -3 times the real one, which has no zero."""
    rng = np.random.default_rng(5)
    o = types.SimpleNamespace()
    o.shape = (M_ROWS, N_COLS)
    o.rowptr, o.colind = exact_pattern(M_ROWS, N_COLS, 6, 24, seed=1)
    o.nnz = int(o.colind.size)
    assert np.bincount(o.colind, minlength=N_COLS).min() >= 1 and np.bincount(o.colind).max() < 100
    o.values = rng.choice([1.0, 2.0], o.nnz)
    o.values_im = rng.choice([1.0, 2.0], o.nnz)
    o.x = rng.choice([1.0, 2.0, 3.0], N_COLS)
    o.x_im = rng.choice([1.0, 2.0], N_COLS)
    o.xt = rng.choice([1.0, 2.0, 3.0], M_ROWS)           # the vector of the transposed product
    o.B = rng.choice([1.0, 2.0, 3.0], (N_COLS, max(NB)))
    o.B_im = rng.choice([1.0, 2.0], (N_COLS, max(NB)))
    return o


@functools.lru_cache(maxsize=None)
def spgemm_operands():
    """A (2000 x 1500), B (1500 x 1800), D (2000 x 1800, the addend), 6 ... 12 entries per row, values 1 or 2: every entry of
    A B (+ D) is a positive integer below 2^10."""
    rng = np.random.default_rng(9)
    g = types.SimpleNamespace()
    g.a_shape, g.b_shape, g.d_shape = (2000, 1500), (1500, 1800), (2000, 1800)
    g.a_rowptr, g.a_colind = exact_pattern(2000, 1500, 6, 12, seed=11)
    g.b_rowptr, g.b_colind = exact_pattern(1500, 1800, 6, 12, seed=12)
    g.d_rowptr, g.d_colind = exact_pattern(2000, 1800, 6, 12, seed=13)
    g.a_values = rng.choice([1.0, 2.0], g.a_colind.size)
    g.b_values = rng.choice([1.0, 2.0], g.b_colind.size)
    g.d_values = rng.choice([1.0, 2.0], g.d_colind.size)
    # the second summand of add(): A's shape
    g.e_rowptr, g.e_colind = exact_pattern(2000, 1500, 6, 12, seed=14)
    g.e_values = rng.choice([1.0, 2.0], g.e_colind.size)
    return g


TRI_WIDTHS = [1500, 300, 40, 3, 3, 200, 130, 3, 150]      # wide and narrow levels, runs of narrow ones: 2329 rows


@functools.lru_cache(maxsize=None)
def tri_system(upper, unit):
    """The exact triangular family of tests/ladder_tt.py (x_true known by construction) on levels of both kinds."""
    return TT.trsv_system(TRI_WIDTHS, [TT.Shape(1), TT.Shape(2), TT.Shape(3, (0,))], 4, upper=upper, unit=unit,
                          seed=31 + 2 * upper + unit, alpha=1.0)


@functools.lru_cache(maxsize=None)
def sweep_system():
    return SW.dyadic_system(2000, 4, seed=41)


ILU_WIDTHS = [600, 400, 300, 3, 2, 300, 200, 195]


@functools.lru_cache(maxsize=None)
def ilu_system():
    """(rowptr, colind, A real, LU real, A decoy, LU decoy) on one pattern: the exact family of ilu_util.exact_system, and a
    second member of it whose factor differs from the first in every entry (L negated, U doubled)."""
    rowptr, colind, _ = IU.level_pattern(ILU_WIDTHS, seed=51)
    a, lu = IU.exact_system(rowptr, colind, seed=52)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    lu2 = np.where(colind < rows, -lu, 2.0 * lu)
    L, U = IU.split_lu(rowptr, colind, lu2)
    a2 = IU._at_pattern(L @ U, rowptr, colind)
    assert np.abs(a2).max() < 2 ** 20 and np.array_equal(a2 * 2, np.round(a2 * 2)), "the decoy leaves the exact range"
    return rowptr, colind, a, lu, a2, lu2


@functools.lru_cache(maxsize=None)
def permute_system():
    rng = np.random.default_rng(61)
    rowptr, colind = MC.random_rows(2000, 8, seed=62)
    perm = rng.permutation(2000).astype(np.int32)
    values = rng.choice([1.0, 2.0, 3.0, 5.0], colind.size) * rng.choice([-1.0, 1.0], colind.size)
    vec = rng.choice([1.0, 2.0, 3.0, 5.0], 2000)
    return rowptr, colind, perm, values, vec


# ===================================================================================================================== cases
class Case:
    """One op form.  Host side: inputs(which) -> {name: float64 / complex128 / int array}, expected(inputs) -> [one array per
    output], violations(got, want), separated(a, b).  Device side: build() -> state (structure, plans, buffers holding the
    DECOYS; all inspect-class work done on the current stream), run(state), results(state)."""
    covers = ()              # the exported names whose launches the late-input test orders
    uses = ()                # ... and the inspect-class names build() runs for it
    late = ()                # the inputs written late
    dtype = torch.float32
    sync = frozenset()       # the variants in which the call is inspect-class
    why = ""                 # ... and why
    compare = "bit for bit (sweeps_util.bit_violations)"
    owner = None             # part B: what owns device arrays here (None: no lifetime test on this case)
    env = {}                 # environment knobs held while build() and run() execute
    value_outputs = None     # indices of the outputs separated() looks at (None: all)

    def __init__(self, name, **kw):
        self.name = name
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return self.name

    # ---- host
    def inputs(self, which):
        raise NotImplementedError

    def expected(self, inputs):
        raise NotImplementedError

    def violations(self, got, want):
        out = []
        if len(got) != len(want):
            return [f"{len(got)} outputs, {len(want)} expected"]
        for i, (g, w) in enumerate(zip(got, want)):
            out += bit_violations(g, w, f"{self.name} output {i}")
        return out

    def separated(self, a, b):
        """True iff the two results differ in every element of every value output."""
        idx = range(len(a)) if self.value_outputs is None else self.value_outputs
        return all(bool((_flat(a[i]) != _flat(b[i])).all()) and _flat(a[i]).size > 0 for i in idx)

    # ---- device
    def cast(self, name):
        """The device dtype of input `name` (None: as the host array is)."""
        return self.dtype

    def new_state(self):
        st = types.SimpleNamespace(buf={}, stage={"real": {}, "decoy": {}}, outs=[], pure=[], info=None)
        real, decoy = self.inputs("real"), self.inputs("decoy")
        for k in real:
            if k in self.late:
                st.stage["real"][k], st.stage["decoy"][k] = to_dev(real[k], self.cast(k)), to_dev(decoy[k], self.cast(k))
                st.buf[k] = torch.empty_like(st.stage["decoy"][k])
            else:                       # an input that is never written late: in place from the start, never touched again
                assert np.array_equal(real[k], decoy[k])
                st.buf[k] = to_dev(real[k], self.cast(k))
        return st

    def out(self, st, shape, dtype=None, pure=True):
        t = torch.empty(shape, dtype=self.dtype if dtype is None else dtype, device="cuda")
        st.outs.append(t)
        if pure:
            st.pure.append(t)
        return t

    def load(self, st, which):
        """Current stream: the `which` inputs into the live buffers, the prefill into the pure outputs."""
        for k in self.late:
            st.buf[k].copy_(st.stage[which][k])
        for t in st.pure:
            prefill(t)

    def late_copies(self, st):
        for k in self.late:
            st.buf[k].copy_(st.stage["real"][k])

    def build(self):
        raise NotImplementedError

    def run(self, st):
        raise NotImplementedError

    def results(self, st):
        return [t.clone() for t in st.outs]

    def after(self, st):
        """Checks that need the op finished (run under the side stream, after it was synchronised)."""

    def drop(self, st):
        """Part B: drops the last reference to the owner."""
        st.info = None


def _csr(st, o, values="values", colind64=False):
    ci = to_dev(o.colind.astype(np.int64 if colind64 else np.int32))
    return sp.csr_view(st.buf[values], to_dev(o.rowptr), ci, o.shape, o.nnz)


class Spmv(Case):
    """y = alpha op(A) x in every form multiply offers for a vector."""
    covers = ("multiply",)
    late = ("values", "x")
    alg = None               # None: plan-free
    form = "csr"             # csr, transposed (transposed(csr)), csc (csc_view), scaled, int64, matrix_opt, prepared
    conj = False

    def inputs(self, which):
        o = operand()
        t = self.form in ("transposed", "csc")
        v, x = o.values, (o.xt if t else o.x)
        if self.dtype.is_complex:
            v, x = v + 1j * o.values_im, x + 1j * o.x_im
        k = (3.0, -1.0) if which == "decoy" else (1.0, 1.0)
        out = {"values": v * k[0], "x": x * k[1]}
        if "values" not in self.late:
            out["values"] = v
        return out

    def expected(self, inputs):
        o = operand()
        v, x = inputs["values"], inputs["x"]
        if self.dtype.is_complex:        # tests/test_gpu_complex.py: scipy in complex128
            A = sps.csr_matrix((np.conj(v) if self.conj else v, o.colind, o.rowptr), shape=o.shape)
            return [A @ x]
        if self.form in ("transposed", "csc"):
            return [oracle.spmv_csc((N_COLS, M_ROWS), o.rowptr, o.colind, v, x)]
        return [oracle.spmv(o.shape, o.rowptr, o.colind, v, x, scale_a=2.0 if self.form == "scaled" else None)]

    def build(self):
        o = operand()
        st = self.new_state()
        wide = self.form == "int64"
        a = _csr(st, o, colind64=wide)
        t = self.form in ("transposed", "csc")
        if self.form == "transposed":
            st.a = sp.transposed(a)
        elif self.form == "csc":
            st.a = sp.csc_view(a.values(), a.rowptr(), a.colind(), (N_COLS, M_ROWS), o.nnz)
        elif self.form == "matrix_opt":
            st.a = sp.matrix_opt(a)
        else:
            st.a = a
        st.y = self.out(st, (N_COLS if t else M_ROWS,))
        if self.alg is not None:
            st.info = sp.multiply_inspect(st.a, st.buf["x"], st.y, alg=self.alg)
            if self.form == "matrix_opt":
                assert st.info.state_.snapshot, "the matrix_opt case needs the plan that keeps a copy of the values"
        st.op = sp.scaled(2.0, st.a) if self.form == "scaled" else sp.conjugated(st.a) if self.conj else st.a
        return st

    def run(self, st):
        if self.form == "prepared":
            sp.prepared_multiply(st.info, st.op, st.buf["x"], st.y)()
        elif st.info is not None:
            sp.multiply(st.info, st.op, st.buf["x"], st.y)
        else:
            sp.multiply(st.op, st.buf["x"], st.y)

    def after(self, st):
        if self.form in ("transposed", "csc"):
            want = "two_pass" if self.env.get("SPBLAS_GFX950_SPMV_T2") == "1" else "scatter"
            got = _Handle.current(st.y.device).spmv_t_last(with_items=False)["path"]
            assert got == want, f"{self.name}: the transposed multiply took the {got} path"

    def drop(self, st):
        st.info = None
        if self.form == "matrix_opt":
            st.a._plan = None
            st.op = st.a = None


class Spmm(Case):
    """C = A B for a dense B of NB columns, row- or column-major."""
    covers = ("multiply",)
    late = ("values", "B")
    n = 3
    inspected = False
    layout_left = False

    def inputs(self, which):
        o = operand()
        v, B = o.values, o.B[:, :self.n]
        if self.dtype.is_complex:
            v, B = v + 1j * o.values_im, B + 1j * o.B_im[:, :self.n]
        k = (3.0, -1.0) if which == "decoy" else (1.0, 1.0)
        return {"values": v * k[0], "B": np.ascontiguousarray(B * k[1])}

    def expected(self, inputs):
        o = operand()
        if self.dtype.is_complex:
            return [sps.csr_matrix((inputs["values"], o.colind, o.rowptr), shape=o.shape) @ inputs["B"]]
        return [oracle.spmm(o.shape, o.rowptr, o.colind, inputs["values"], inputs["B"])]

    def new_state(self):
        st = super().new_state()
        if self.layout_left:     # the live B is column-major: a transposed view of an (n, k) buffer; the stages stay row-major
            st.buf["B"] = torch.empty((self.n, N_COLS), dtype=self.dtype, device="cuda").t()
        return st

    def build(self):
        o = operand()
        st = self.new_state()
        st.a = _csr(st, o)
        st.c = self.out(st, (M_ROWS, self.n))
        if self.inspected:
            st.info = sp.multiply_inspect(st.a, st.buf["B"], st.c)
        return st

    def run(self, st):
        if st.info is not None:
            sp.multiply(st.info, st.a, st.buf["B"], st.c)
        else:
            sp.multiply(st.a, st.buf["B"], st.c)


class Spgemm(Case):
    """C = A B (+ D): multiply_compute in build(), the fill under test.  prior = numeric passes build() has already run on the
    state: 0 the one-shot fill, 1 the fill that records the ranks, 2 the fill by rank."""
    late = ("a_values", "b_values")
    prior = 0
    addend = False
    state_api = False        # spgemm_state_t with multiply_symbolic_compute / multiply_symbolic_fill / multiply_numeric
    value_outputs = (0,)

    def inputs(self, which):
        g = spgemm_operands()
        k = (3.0, -1.0, -3.0) if which == "decoy" else (1.0, 1.0, 1.0)
        out = {"a_values": g.a_values * k[0], "b_values": g.b_values * k[1]}
        if self.addend:
            out["d_values"] = g.d_values * k[2]
        return out

    def expected(self, inputs):
        g = spgemm_operands()
        if self.addend:
            n, _ = oracle.spgemm_symbolic_d(g.a_shape, g.a_rowptr, g.a_colind, g.b_shape, g.b_rowptr, g.b_colind, g.d_shape,
                                            g.d_rowptr, g.d_colind)
            rp, ci, v = oracle.spgemm_numeric_d(g.a_shape, g.a_rowptr, g.a_colind, inputs["a_values"], g.b_shape, g.b_rowptr,
                                                g.b_colind, inputs["b_values"], g.d_shape, g.d_rowptr, g.d_colind,
                                                inputs["d_values"], capacity=n)
        else:
            n, _ = oracle.spgemm_symbolic(g.a_shape, g.a_rowptr, g.a_colind, g.b_shape, g.b_rowptr, g.b_colind)
            rp, ci, v = oracle.spgemm_numeric(g.a_shape, g.a_rowptr, g.a_colind, inputs["a_values"], g.b_shape, g.b_rowptr,
                                              g.b_colind, inputs["b_values"], capacity=n)
        return [v, ci, rp]

    def build(self):
        g = spgemm_operands()
        st = self.new_state()
        st.a = sp.csr_view(st.buf["a_values"], to_dev(g.a_rowptr), to_dev(g.a_colind), g.a_shape, g.a_colind.size)
        st.b = sp.csr_view(st.buf["b_values"], to_dev(g.b_rowptr), to_dev(g.b_colind), g.b_shape, g.b_colind.size)
        st.d = sp.csr_view(st.buf["d_values"], to_dev(g.d_rowptr), to_dev(g.d_colind), g.d_shape, g.d_colind.size) \
            if self.addend else None
        m, n = g.a_shape[0], g.b_shape[1]
        c_rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        st.c = sp.csr_view(None, c_rp, None, (m, n), 0)
        extra = (st.d,) if self.addend else ()
        if self.state_api:
            st.info = sp.spgemm_state_t()
            sp.multiply_symbolic_compute(st.info, st.a, st.b, st.c, *extra)
            nnz = st.info.result_nnz()
        else:
            st.info = sp.multiply_compute(st.a, st.b, st.c)
            nnz = st.info.result_nnz()
        st.c_values = self.out(st, (nnz,))
        st.c_colind = self.out(st, (nnz,), torch.int32)
        st.outs.append(c_rp)           # written by every fill from the state's copy; not prefilled (compute wrote it too)
        st.c.update(st.c_values, c_rp, st.c_colind, (m, n), nnz)
        st.extra = extra
        self.load(st, "decoy")
        for i in range(self.prior):
            if self.state_api and i == 0:
                sp.multiply_symbolic_fill(st.info, st.a, st.b, st.c, *extra)
            else:
                self.run(st)
        if self.prior >= 2:
            torch.cuda.synchronize()
            assert st.info.info()["fills_by_rank"] if self.state_api else st.info.state_.info()["fills_by_rank"], \
                "the third fill was to go by rank"
        return st

    def run(self, st):
        if self.state_api:
            sp.multiply_numeric(st.info, st.a, st.b, st.c, *st.extra)
        else:
            sp.multiply_fill(st.info, st.a, st.b, st.c)


class Add(Case):
    """C = A + E: add_inspect in build() and add_compute under test, or add() in one call."""
    late = ("a_values", "e_values")
    one_shot = False
    value_outputs = (0,)

    def inputs(self, which):
        g = spgemm_operands()
        k = -3.0 if which == "decoy" else 1.0
        return {"a_values": g.a_values * k, "e_values": g.e_values * k}

    def expected(self, inputs):
        g = spgemm_operands()
        rp, ci, v = oracle.add(g.a_shape, g.a_rowptr, g.a_colind, inputs["a_values"], g.a_shape, g.e_rowptr, g.e_colind,
                               inputs["e_values"])
        return [v, ci, rp]

    def build(self):
        g = spgemm_operands()
        st = self.new_state()
        st.a = sp.csr_view(st.buf["a_values"], to_dev(g.a_rowptr), to_dev(g.a_colind), g.a_shape, g.a_colind.size)
        st.b = sp.csr_view(st.buf["e_values"], to_dev(g.e_rowptr), to_dev(g.e_colind), g.a_shape, g.e_colind.size)
        nnz = int(oracle.add(g.a_shape, g.a_rowptr, g.a_colind, g.a_values, g.a_shape, g.e_rowptr, g.e_colind, g.e_values,
                             symbolic=True)[0])
        st.nnz = nnz
        st.c_values = self.out(st, (nnz,))
        st.c_colind = self.out(st, (nnz,), torch.int32)
        st.c_rowptr = self.out(st, (g.a_shape[0] + 1,), torch.int32)
        st.c = sp.csr_view(st.c_values, st.c_rowptr, st.c_colind, g.a_shape, nnz)
        if not self.one_shot:
            st.info = sp.add_inspect(st.a, st.b, st.c)
            assert st.info.result_nnz() == nnz
            st.pure = [t for t in st.pure if t is not st.c_rowptr]     # written by the inspect: the compute copies it again
        return st

    def run(self, st):
        if self.one_shot:
            sp.add(st.a, st.b, st.c)
        else:
            sp.add_compute(st.info, st.a, st.b, st.c)


class Transpose(Case):
    covers = ("transpose",)
    uses = ("transpose_inspect",)
    late = ("values",)
    sync = frozenset({"fresh"})
    why = "takes the handle's grow-only scratch: the first call of a size frees the smaller buffer (hipFree waits)"
    value_outputs = (0,)

    def inputs(self, which):
        return {"values": operand().values * (-3.0 if which == "decoy" else 1.0)}

    def expected(self, inputs):
        o = operand()
        rp, ci, v = oracle.transpose(o.shape, o.rowptr, o.colind, inputs["values"])
        return [v, ci, rp]

    def build(self):
        o = operand()
        st = self.new_state()
        st.a = _csr(st, o)
        v, ci, rp = self.out(st, (o.nnz,)), self.out(st, (o.nnz,), torch.int32), self.out(st, (N_COLS + 1,), torch.int32)
        st.b = sp.csr_view(v, rp, ci, (N_COLS, M_ROWS), o.nnz)
        st.tinfo = sp.transpose_inspect(st.a, st.b)
        return st

    def run(self, st):
        sp.transpose(st.tinfo, st.a, st.b)


class Scale(Case):
    """scale(2, t) in place: a vector, and the values of a matrix view."""
    covers = ("scale",)
    late = ("t",)
    matrix = False

    def inputs(self, which):
        o = operand()
        return {"t": (o.values if self.matrix else o.xt) * (-3.0 if which == "decoy" else 1.0)}

    def expected(self, inputs):
        return [2.0 * inputs["t"]]

    def build(self):
        st = self.new_state()
        st.outs.append(st.buf["t"])
        st.t = _csr(st, operand(), values="t") if self.matrix else st.buf["t"]
        return st

    def run(self, st):
        sp.scale(2.0, st.t)


class Trsv(Case):
    """triangular_solve on the exact family: vector or block of three right-hand sides; the cooperative solve or one launch per
    level (the switch of test_alternative_inspect_and_solve_paths, read by the inspect)."""
    covers = ("triangular_solve",)
    uses = ("triangular_solve_inspect",)
    late = ("values", "b")
    upper, unit, block = False, True, False
    owner = "the level plan of triangular_solve_inspect"
    compare = "bit for bit against x_true (ladder_tt.exact_violations)"

    def sysm(self):
        return tri_system(self.upper, self.unit)

    def factor(self, which):
        """decoy: b times -2, and the stored values doubled where the diagonal is stored: x is -x_true (unit: -2 x_true)."""
        return 1.0 if which == "real" else (-2.0 if self.unit else -1.0)

    def inputs(self, which):
        y = self.sysm()
        b = TT.block_rhs(y) if self.block else y.b
        if which == "real":
            return {"values": y.exact_values, "b": b}
        return {"values": y.exact_values * (1.0 if self.unit else 2.0), "b": -2.0 * b}

    def expected(self, inputs):
        y = self.sysm()
        which = "real" if np.array_equal(inputs["b"], self.inputs("real")["b"]) else "decoy"
        x = y.x_true * self.factor(which)
        return [np.stack([x * f for f in TT.BLOCK_FACTORS], axis=1) if self.block else x]

    def build(self):
        y = self.sysm()
        st = self.new_state()
        st.a = sp.csr_view(st.buf["values"], to_dev(y.rowptr), to_dev(y.colind), (y.m, y.m), y.nnz)
        st.x = self.out(st, (y.m, 3) if self.block else (y.m,))
        st.tri = (sp.upper_triangle if self.upper else sp.lower_triangle,
                  sp.implicit_unit_diagonal if self.unit else sp.explicit_diagonal)
        st.info = sp.triangular_solve_inspect(st.a, *st.tri, st.buf["b"], st.x)
        launches = st.info.state_.info()["launches_per_solve"]
        if self.env.get("SPBLAS_GFX950_TRSV_COOP") == "0":
            assert launches > 1, "the launch-per-level plan was asked for"
        elif not (os.environ.get("ROCP_TOOL_LIBRARIES") or os.environ.get("HSA_TOOLS_LIB")):
            assert launches == 1, "the cooperative solve was expected"
        return st

    def run(self, st):
        sp.triangular_solve(st.info, st.a, *st.tri, st.buf["b"], st.x)


class Sweeps(Case):
    """triangular_solve_sweeps, three sweeps on the dyadic family, with the level plan and plan-free."""
    covers = ("triangular_solve_sweeps",)
    late = ("values", "b")
    planned = True
    sweeps = 3
    compare = "bit for bit against sweeps_util.reference"

    def inputs(self, which):
        y = sweep_system()
        # decoy: b plus a large random integer per row.  The iterates are linear in b; small regular shifts cancel in a few rows
        # of this small-integer family (k b + c for a dozen (k, c) left 8 ... 85 equal elements), these do not (host-checked)
        shift = np.random.default_rng(43).integers(1000, 5000, y.m).astype(np.float64)
        return {"values": y.values, "b": y.b if which == "real" else y.b + shift}

    def expected(self, inputs):
        y = sweep_system()
        return [SW.host_sweeps(y.rowptr, y.colind, inputs["values"], inputs["b"], self.sweeps, y.uplo, y.diag, y.alpha,
                               np.float32)[0]]

    def build(self):
        y = sweep_system()
        st = self.new_state()
        st.a = sp.csr_view(st.buf["values"], to_dev(y.rowptr), to_dev(y.colind), (y.m, y.m), y.nnz)
        st.x = self.out(st, (y.m,))
        st.tri = (sp.upper_triangle if y.uplo == "upper" else sp.lower_triangle,
                  sp.implicit_unit_diagonal if y.diag == "unit" else sp.explicit_diagonal)
        st.op = st.a if y.alpha == 1.0 else sp.scaled(y.alpha, st.a)
        if self.planned:
            st.info = sp.triangular_solve_inspect(st.a, *st.tri, st.buf["b"], st.x)
        return st

    def run(self, st):
        if st.info is not None:
            sp.triangular_solve_sweeps(st.info, st.op, *st.tri, st.buf["b"], st.x, self.sweeps)
        else:
            sp.triangular_solve_sweeps(st.op, *st.tri, st.buf["b"], st.x, self.sweeps)


class Ilu0(Case):
    """ilu0 out of place and in place, ilu0_sweeps at its fixed point (the sweep count is clamped to levels - 1, where the
    result IS ilu0): the exact family, late values of A, ilu0_status read afterwards."""
    uses = ("ilu0_inspect", "ilu0_status")
    late = ("a",)
    inplace = False
    by_sweeps = False
    compare = "bit for bit against the factor the family was built from (ilu_util.exact_violations)"

    def inputs(self, which):
        _, _, a, _, a2, _ = ilu_system()
        return {"a": a if which == "real" else a2}

    def expected(self, inputs):
        _, _, a, lu, _, lu2 = ilu_system()
        return [lu if np.array_equal(inputs["a"], a) else lu2]

    def violations(self, got, want):
        rowptr, colind = ilu_system()[:2]
        return IU.exact_violations(got[0], want[0], rowptr, colind)

    def build(self):
        rowptr, colind = ilu_system()[:2]
        m, nnz = rowptr.size - 1, colind.size
        st = self.new_state()
        rp, ci = to_dev(rowptr), to_dev(colind)
        st.a = sp.csr_view(st.buf["a"], rp, ci, (m, m), nnz)
        if self.inplace:
            st.lu = st.a
            st.outs.append(st.buf["a"])
        else:
            st.lu = sp.csr_view(self.out(st, (nnz,)), rp, ci, (m, m), nnz)
        st.work = torch.empty(nnz, dtype=self.dtype, device="cuda") if self.by_sweeps else None
        st.info = sp.ilu0_inspect(st.a)
        return st

    def run(self, st):
        if self.by_sweeps:
            sp.ilu0_sweeps(st.info, st.a, st.lu, st.work, 2 ** 30)
        else:
            sp.ilu0(st.info, st.a, st.lu)

    def after(self, st):
        assert sp.ilu0_status(st.info) == -1, f"{self.name}: a pivot of the exact family was reported"


class GaussSeidel(Case):
    """gauss_seidel, two sweeps on the dyadic family (A with its perm), late b and late incoming x, x in place."""
    covers = ("gauss_seidel",)
    uses = ("gauss_seidel_inspect",)
    late = ("b", "x")
    omega, direction = 1.0, "forward"
    owner = "the plan of gauss_seidel_inspect"
    compare = "bit for bit against gs_util.reference"

    def inputs(self, which):
        y = GS.dyadic_system(4)
        if which == "real":
            return {"b": y.b, "x": y.x0}
        # decoy: x0 + 1 and b + A 1: every iterate of the sweep is the real one plus 1 (the shift is a fixed point of the update)
        A = sps.csr_matrix((y.values, y.colind, y.rowptr), shape=(y.m, y.m))
        return {"b": y.b + A @ np.ones(y.m), "x": y.x0 + 1.0}

    def expected(self, inputs):
        y = GS.dyadic_system(4)
        return [GS.host_gauss_seidel(y.rowptr, y.colind, y.values, inputs["b"], inputs["x"], y.color_ptr, y.perm, 2, self.omega,
                                     self.direction, np.float32)[0]]

    def build(self):
        y = GS.dyadic_system(4)
        st = self.new_state()
        st.a = sp.csr_view(to_dev(y.values, self.dtype), to_dev(y.rowptr), to_dev(y.colind), (y.m, y.m), y.nnz)
        st.outs.append(st.buf["x"])
        st.info = sp.gauss_seidel_inspect(st.a, to_dev(y.color_ptr), perm=to_dev(y.perm))
        return st

    def run(self, st):
        sp.gauss_seidel(st.info, st.a, st.buf["b"], st.buf["x"], sweeps=2, omega=self.omega, direction=self.direction)


class Permute(Case):
    """permute: the value gather of an inspected permutation, and the one-call form that inspects first."""
    covers = ("permute",)
    late = ("values",)
    inspected = True
    owner = "the plan of permute_inspect"
    value_outputs = (0,)

    def inputs(self, which):
        return {"values": permute_system()[3] * (-3.0 if which == "decoy" else 1.0)}

    def expected(self, inputs):
        rowptr, colind, perm = permute_system()[:3]
        b_rp, b_ci, pos = MC.host_permute(rowptr, colind, perm)
        return [inputs["values"][pos], b_ci, b_rp]

    def build(self):
        rowptr, colind, perm = permute_system()[:3]
        m, nnz = rowptr.size - 1, colind.size
        st = self.new_state()
        st.a = sp.csr_view(st.buf["values"], to_dev(rowptr), to_dev(colind), (m, m), nnz)
        st.perm = to_dev(perm)
        # (the structure of B is written by the inspect: prefilled only where the call under test inspects)
        v = self.out(st, (nnz,))
        ci = self.out(st, (nnz,), torch.int32, pure=not self.inspected)
        rp = self.out(st, (m + 1,), torch.int32, pure=not self.inspected)
        st.b = sp.csr_view(v, rp, ci, (m, m), nnz)
        if self.inspected:
            st.info = sp.permute_inspect(st.a, st.perm, st.b)
        return st

    def run(self, st):
        if self.inspected:
            sp.permute(st.info, st.a, st.perm, st.b)
        else:
            sp.permute(st.a, st.perm, st.b)


class PermuteVector(Case):
    covers = ("permute_vector",)
    late = ("src",)
    inverse = False

    def inputs(self, which):
        return {"src": permute_system()[4] * (-3.0 if which == "decoy" else 1.0)}

    def expected(self, inputs):
        perm = permute_system()[2]
        if not self.inverse:
            return [inputs["src"][perm]]
        out = np.empty_like(inputs["src"])
        out[perm] = inputs["src"]
        return [out]

    def build(self):
        st = self.new_state()
        st.perm = to_dev(permute_system()[2])
        st.dst = self.out(st, (st.perm.numel(),))
        return st

    def run(self, st):
        sp.permute_vector(st.perm, st.buf["src"], st.dst, inverse=self.inverse)


class Multicolor(Case):
    """multicolor_order reads structure only: its late input is the column array, written late from a staged copy of a valid
    pattern over another valid pattern on the same row offsets (every row's columns replaced by its own index: a graph
    without edges, one colour).  Both are in range for the same m.  The four result arrays are allocated by the call; a decoy
    result differs from the real one as a whole, not in every element (colour 0 exists in both)."""
    covers = ("multicolor_order",)
    late = ("colind",)
    sync = frozenset(VARIANTS)
    why = "inspect-class: allocates, reads the colour counts back, synchronises"
    compare = "array_equal against multicolor_util.model_colors / order_from_colors"

    def pattern(self):
        return MC.random_rows(2000, 8, seed=71)

    def inputs(self, which):
        rowptr, colind = self.pattern()
        rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr)).astype(np.int32)
        return {"colind": colind if which == "real" else rows}

    def cast(self, name):
        return torch.int32

    def expected(self, inputs):
        rowptr = self.pattern()[0]
        color = MC.model_colors(rowptr, inputs["colind"])
        perm, inverse, color_ptr = MC.order_from_colors(color)
        return [perm, inverse, color, color_ptr]

    def separated(self, a, b):
        return all(a[i].shape != b[i].shape or not np.array_equal(a[i], b[i]) for i in range(4))

    def build(self):
        rowptr, colind = self.pattern()
        m = rowptr.size - 1
        st = self.new_state()
        st.a = sp.csr_view(torch.ones(colind.size, device="cuda"), to_dev(rowptr), st.buf["colind"], (m, m), colind.size)
        return st

    def run(self, st):
        st.order = sp.multicolor_order(st.a)

    def results(self, st):
        o = st.order
        return [o.perm.clone(), o.inverse.clone(), o.color.clone(), o.color_ptr.clone()]


T2 = "SPBLAS_GFX950_SPMV_T2"           # the knob of tests/ladder_t2.py: 1 forces the two-pass transposed multiply, 0 the scatter
COOP = "SPBLAS_GFX950_TRSV_COOP"
SCRATCH = "takes the handle's grow-only scratch: the first call of a size frees the smaller buffer (hipFree waits)"
REFRESH = "the plan's copy of the values is refreshed first (update_values: inspect-class, refused inside a capture)"
NARROW = "the int64 columns are narrowed and range-checked on the first call: the answer is read back (synchronises)"
SYMBOLIC = "the symbolic pass reads nnz(C) back: the one wait the API asks for"
RECORD = "the second fill of a symbolic result records the ranks: sizes them on the host (synchronises)"
ALL = frozenset(VARIANTS)


def _cases():
    A = _capi
    c = [
        Spmv("spmv_plan_free"),
        Spmv("spmv_auto", alg=A.SPMV_AUTO, uses=("multiply_inspect",)),
        Spmv("spmv_vector", alg=A.SPMV_VECTOR, uses=("multiply_inspect",)),
        Spmv("spmv_rowblock", alg=A.SPMV_ROWBLOCK, uses=("multiply_inspect",), owner="the SpMV plan of multiply_inspect"),
        Spmv("spmv_sliced", alg=A.SPMV_SLICED, late=("x",), uses=("multiply_inspect",)),
        Spmv("spmv_matrix_opt_snapshot", alg=A.SPMV_SLICED, form="matrix_opt", sync=ALL, why=REFRESH,
             covers=("multiply", "matrix_opt"), uses=("multiply_inspect",)),
        Spmv("spmv_prepared", alg=A.SPMV_ROWBLOCK, form="prepared", covers=("prepared_multiply",), uses=("multiply_inspect",)),
        Spmv("spmv_transposed_scatter", form="transposed", env={T2: "0"}, covers=("multiply", "transposed")),
        Spmv("spmv_csc_scatter", form="csc", env={T2: "0"}, covers=("multiply", "csc_view")),
        Spmv("spmv_transposed_two_pass", form="transposed", env={T2: "1"}, sync=frozenset({"fresh"}), why=SCRATCH,
             covers=("multiply", "transposed")),
        Spmv("spmv_csc_two_pass", form="csc", env={T2: "1"}, sync=frozenset({"fresh"}), why=SCRATCH,
             covers=("multiply", "csc_view")),
        Spmv("spmv_scaled", form="scaled", covers=("multiply", "scaled")),
        Spmv("spmv_int64_columns", form="int64", sync=frozenset({"fresh"}), why=NARROW),
        Spmv("spmv_int64_columns_rowblock", form="int64", alg=A.SPMV_ROWBLOCK, uses=("multiply_inspect",)),
        Spmv("spmv_bf16", dtype=torch.bfloat16, compare="bit for bit (ladder.bits_equal)"),
        Spmv("spmv_fp16", dtype=torch.float16, compare="bit for bit (ladder.bits_equal)"),
        Spmv("spmv_bf16_rowblock", dtype=torch.bfloat16, alg=A.SPMV_ROWBLOCK, uses=("multiply_inspect",),
             compare="bit for bit (ladder.bits_equal)"),
        Spmv("spmv_complex64", dtype=torch.complex64),
        Spmv("spmv_complex64_conjugated", dtype=torch.complex64, conj=True, covers=("multiply", "conjugated")),
        Spmm("spmm_plan_free_n3"),
        Spmm("spmm_inspected_n3", inspected=True, uses=("multiply_inspect",), owner="the SpMM plan of multiply_inspect"),
        Spmm("spmm_plan_free_n64", n=64),
        Spmm("spmm_inspected_n64", n=64, inspected=True, uses=("multiply_inspect",)),
        Spmm("spmm_layout_left_n3", layout_left=True),
        Spmm("spmm_bf16_n3", dtype=torch.bfloat16, compare="bit for bit (ladder.bits_equal)"),
        Spmm("spmm_complex64_n3", dtype=torch.complex64),
        Spgemm("spgemm_fill_one_shot", covers=("multiply_fill",), uses=("multiply_compute",), sync=frozenset({"warmed"}),
               why=RECORD, owner="the SpGEMM state of multiply_compute"),
        Spgemm("spgemm_fill_recording", prior=1, covers=("multiply_fill",), uses=("multiply_compute",),
               sync=frozenset({"fresh"}), why=RECORD),
        Spgemm("spgemm_fill_by_rank", prior=2, state_api=True, covers=("multiply_numeric",),
               uses=("multiply_symbolic_compute", "multiply_symbolic_fill", "spgemm_state_t")),
        Spgemm("spgemm_numeric_with_addend", prior=1, state_api=True, addend=True, late=("a_values", "b_values", "d_values"),
               covers=("multiply_numeric",), uses=("multiply_symbolic_compute", "multiply_symbolic_fill", "spgemm_state_t"),
               sync=frozenset({"fresh"}), why=RECORD),
        Add("add_compute", covers=("add_compute",), uses=("add_inspect",), sync=frozenset({"warmed"}), why=RECORD),
        Add("add_one_shot", one_shot=True, covers=("add",), sync=ALL, why=SYMBOLIC),
        Transpose("transpose"),
        Scale("scale_vector"),
        Scale("scale_matrix_values", matrix=True),
    ]
    for upper, unit in ((False, True), (True, False)):
        tag = ("upper" if upper else "lower") + ("_unit" if unit else "_explicit")
        c += [Trsv(f"trsv_{tag}_cooperative", upper=upper, unit=unit),
              Trsv(f"trsv_{tag}_launch_per_level", upper=upper, unit=unit, env={COOP: "0"}, owner=None),
              Trsv(f"trsm_{tag}_block3", upper=upper, unit=unit, block=True, env={COOP: "0"})]
    c += [
        Sweeps("sweeps_with_level_plan", uses=("triangular_solve_inspect",), owner="the level plan the sweeps walk"),
        Sweeps("sweeps_plan_free", planned=False),
        Ilu0("ilu0_out_of_place", covers=("ilu0",), owner="the plan of ilu0_inspect"),
        Ilu0("ilu0_in_place", covers=("ilu0",), inplace=True),
        Ilu0("ilu0_sweeps", covers=("ilu0_sweeps",), by_sweeps=True),
        GaussSeidel("gauss_seidel_forward_omega_1"),
        GaussSeidel("gauss_seidel_forward_omega_1.5", omega=1.5, owner=None),
        GaussSeidel("gauss_seidel_symmetric_omega_1", direction="symmetric", owner=None),
        GaussSeidel("gauss_seidel_symmetric_omega_1.5", omega=1.5, direction="symmetric", owner=None),
        Permute("permute_values", uses=("permute_inspect",)),
        Permute("permute_one_call", inspected=False, owner=None, sync=ALL,
                why="without an info the call inspects: allocates, checks perm, synchronises"),
        PermuteVector("permute_vector"),
        PermuteVector("permute_vector_inverse", inverse=True),
        Multicolor("multicolor_order"),
    ]
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Exported names that launch nothing of their own: views and tags, the index type, pure host queries, result holders.
EXEMPT = {
    "csr_view": "a view: holds tensors, launches nothing",
    "scaled_view": "a view class (scaled() builds it)",
    "index": "the index pair type",
    "get_scaling_factor": "host query on views", "get_ultimate_base": "host query on views",
    "has_matrix_opt": "host query on views", "is_conjugated": "host query on views",
    "operation_info_t": "the holder of an inspect result", "multicolor_order_t": "the holder of an ordering",
    "upper_triangle_t": "tag type", "lower_triangle_t": "tag type", "implicit_unit_diagonal_t": "tag type",
    "explicit_diagonal_t": "tag type", "upper_triangle": "tag", "lower_triangle": "tag", "implicit_unit_diagonal": "tag",
    "explicit_diagonal": "tag",
    "BackendError": "the exception type", "generate": "host-side input generators", "_build": "the build module",
    "_capi": "the ctypes binding",
}

# Part C: the cases whose op the test itself issues out of order, to show that part A would see it.
MISORDERED = ("spmv_plan_free", "trsm_lower_unit_block3", "spgemm_fill_one_shot")
