"""-m gpu: the smooth_prolongator calls take their order from the stream the handle is bound to at the call, and the plan frees its
arrays behind its last use -- in the manner of tests/test_gpu_aggregate_stream.py, with the hold / calibration helpers of
tests/stream_util.py used as they are.  The cases are named in smooth_util.STREAM_CASES.

A  late inputs: behind a hold of about 30 ms on a side stream the real inputs (or the poison of an output) are written in stream
   order, then the op runs; the stream must still be busy when the call returns (execute-class: nothing waits) and the result
   must be the real one bit for bit.
B  a plan is dropped while the handle sits on a second stream B and the plan's last use is still pending on A: what B runs
   after the destroy must come after that use.  Control: a probe on B BEFORE the destroy still sees the old contents."""
import gc

import numpy as np
import pytest
import torch

import aggregate_util as A
import gpu_util as G
import ilu_util as U
import smooth_util as M
import spblas_reference_amd as sp
import stream_util as S

pytestmark = pytest.mark.gpu
WILD = 2 ** 30
OMEGA = 2.0 / 3.0


class Tiny:
    """A small unrelated SpMV: calling it re-binds the thread's handle to the current stream."""

    def __init__(self):
        rng = np.random.default_rng(3)
        self.a = sp.csr_view(G.dev(rng.random(80).astype(np.float32)), G.dev((np.arange(11) * 8).astype(np.int32)),
                             G.dev(rng.integers(0, 50, 80).astype(np.int32)), (10, 50), 80)
        self.x, self.y = G.dev(rng.random(50).astype(np.float32)), torch.empty(10, device="cuda")

    def __call__(self):
        sp.multiply(self.a, self.x, self.y)


@pytest.fixture(scope="module")
def streams(gpu):
    S.calibrate()
    out = torch.cuda.Stream(), torch.cuda.Stream()
    tiny = Tiny()
    for s in out:
        with torch.cuda.stream(s):
            tiny()
            torch.zeros(8, device="cuda").clone()
        s.synchronize()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def system(gpu):
    """The 12^3 Laplacian pattern with a diagonal of 64 and small negative integers off it (real), and a decoy of other values:
    every row of the real P differs from the decoy's."""
    rp, ci, lap = A.lap7(12)
    rows = A._rows(rp)
    rng = np.random.default_rng(2)
    real = np.where(ci == rows, 64.0, -rng.integers(1, 9, ci.size).astype(np.float64))
    decoy = np.where(ci == rows, 32.0, 3.0 * real)
    want = A.model(rp, ci, lap)
    ns = type("System", (), {})()
    ns.rp, ns.ci, ns.lap, ns.real, ns.decoy, ns.want = rp, ci, lap, real, decoy, want
    ns.p = M.model(rp, ci, real, want["agg"], want["n_agg"], OMEGA, 0.0, np.float32)
    ns.p_decoy = M.model(rp, ci, decoy, want["agg"], want["n_agg"], OMEGA, 0.0, np.float32)
    assert not np.array_equal(ns.p["p_values"], ns.p_decoy["p_values"])
    return ns


def build(system):
    st = type("State", (), {})()
    nnz = system.ci.size
    st.values = G.dev(system.decoy.astype(np.float32))
    st.stage = G.dev(system.real.astype(np.float32))
    st.a = sp.csr_view(st.values, G.dev(system.rp), G.dev(system.ci), (1728, 1728), nnz)
    n = system.want["n_agg"]
    st.agg = G.dev(system.want["agg"])
    st.info = sp.smooth_prolongator_inspect(st.a, st.agg, n)
    pn = st.info.nnz
    st.p = sp.csr_view(torch.full((pn,), float("nan"), device="cuda"), torch.full((1729,), WILD, dtype=torch.int32, device="cuda"),
                       torch.full((pn,), WILD, dtype=torch.int32, device="cuda"), (1728, n), pn)
    torch.cuda.synchronize()
    return st


def behind_a_hold(stream, late, run):
    """On `stream`: a hold, `late()` behind it in stream order, then run(); returns whether the hold was still in force when
    run() returned."""
    with torch.cuda.stream(stream):
        S.hold(stream)
        e = torch.cuda.Event()
        e.record()
        late()
        run()
        busy = not stream.query() and not e.query()
    return busy


# ============================================================================================================= A: late inputs
def test_smooth_values_late_inputs(streams, system):
    st = build(system)
    for variant in ("fresh", "warmed"):
        if variant == "warmed":
            sp.smooth_prolongator(st.info, st.a, st.p, OMEGA)    # one execute on the default stream first
            torch.cuda.synchronize()
        st.values.copy_(G.dev(system.decoy.astype(np.float32)))
        st.p.values().fill_(float("nan"))
        torch.cuda.synchronize()
        busy = behind_a_hold(streams[0], lambda: st.values.copy_(st.stage),
                             lambda: sp.smooth_prolongator(st.info, st.a, st.p, OMEGA))
        assert busy, "the hold had run out when the call returned: too short, or this execute-class call waited"
        with torch.cuda.stream(streams[0]):
            got = st.p.values().clone()
        streams[0].synchronize()
        assert np.array_equal(U.bits(G.host(got)), U.bits(system.p["p_values"])), variant


def test_smooth_structure_late(streams, system):
    st = build(system)

    def poison():
        st.p.rowptr().fill_(WILD)
        st.p.colind().fill_(WILD)

    busy = behind_a_hold(streams[0], poison, lambda: sp.smooth_prolongator_structure(st.info, st.p))
    assert busy
    streams[0].synchronize()
    assert np.array_equal(G.host(st.p.rowptr()), system.p["p_rowptr"])
    assert np.array_equal(G.host(st.p.colind()), system.p["p_colind"])


# ================================================================================= B: the plan dies behind its last use
def lifetime(streams, outs, use, drop):
    """Steps of part B of tests/test_gpu_stream_order.py: (before, probe0, probe1) as host arrays."""
    A_, B_ = streams
    tiny = Tiny()
    tiny()
    before = [t.clone() for t in outs]
    torch.cuda.synchronize()
    with torch.cuda.stream(A_):
        S.hold(A_)
        use()
    with torch.cuda.stream(B_):
        tiny()                                                  # the handle now sits on B
        probe0 = [t.clone() for t in outs]
    with torch.cuda.stream(B_):
        drop()
        gc.collect()
        probe1 = [t.clone() for t in outs]
    A_.synchronize()
    B_.synchronize()
    raw = lambda t: t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()
    for b, p in zip(before, probe0):
        assert np.array_equal(raw(b), raw(p)), \
            "control: stream B saw the op's output before the destroy -- B was ordered behind A anyway, or the hold had run out"
    return [G.host(t) for t in probe1]


def test_smooth_plan_dies_behind_its_last_use(streams, system):
    """The probe B ran AFTER the destroy holds the value pass's result."""
    st = build(system)
    st.values.copy_(st.stage)
    torch.cuda.synchronize()
    holder = {"info": st.info}
    st.info = None
    probe1 = lifetime(streams, [st.p.values()], lambda: sp.smooth_prolongator(holder["info"], st.a, st.p, OMEGA), holder.clear)
    assert np.array_equal(U.bits(probe1[0]), U.bits(system.p["p_values"])), \
        "what B ran after the destroy was not behind the plan's last use"
