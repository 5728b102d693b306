"""-m gpu: every op takes its order from the stream the handle is bound to at the call, and every owner of device arrays frees
them behind its last use.  The cases, their data and the reasoning are in tests/stream_util.py (proved on the host by
tests/test_stream_order_cpu.py).

A  late inputs: behind a hold of about 30 ms on a side stream the real inputs are copied over decoys in stream order, then the
   op runs; it must return expected(real) bit for bit.  `fresh` is the first execute of the plan (or of the plan-free op),
   `warmed` follows one execute on the default stream, so the handle and the plan were last on another stream and every lazily
   sized workspace exists.
B  the owner of a plan is dropped while the handle sits on a second stream B and the plan's last use is still pending on A:
   what B runs after the destroy must come after that use.
C  the test itself issues three ops on an idle third stream: they return expected(decoy) -- part A would see a stray launch.
"""
import time

import numpy as np
import pytest
import torch

import spblas_reference_amd as sp
import stream_util as S

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def expected(case, which):
    """expected(real) / expected(decoy) of a case, computed once and left unchanged."""
    key = (case.name, which)
    if key not in _EXPECTED:
        _EXPECTED[key] = case.expected(case.inputs(which))
    return _EXPECTED[key]


def host(tensors):
    return [S.to_host(t) for t in tensors]


def raw(t):
    """The bytes of a tensor (NaN compares equal to itself here)."""
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()


@pytest.fixture(scope="module")
def streams(gpu):
    """Three side streams, made once and one after the other, each used once (a stream's first submission sets its queue
    up, which is not what a hold should be spent on), and the filler calibrated."""
    S.calibrate()
    out = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    tiny = Tiny()
    for s in out:
        with torch.cuda.stream(s):
            tiny()
            torch.zeros(8, device="cuda").clone()
        s.synchronize()
    torch.cuda.synchronize()
    return out


class Tiny:
    """A small unrelated SpMV: calling it re-binds the thread's handle to the current stream."""

    def __init__(self):
        rng = np.random.default_rng(3)
        rowptr = (np.arange(11) * 8).astype(np.int32)
        self.a = sp.csr_view(S.to_dev(rng.random(80).astype(np.float32)), S.to_dev(rowptr),
                             S.to_dev(rng.integers(0, 50, 80).astype(np.int32)), (10, 50), 80)
        self.x, self.y = S.to_dev(rng.random(50).astype(np.float32)), torch.empty(10, device="cuda")

    def __call__(self):
        sp.multiply(self.a, self.x, self.y)


# ================================================================================================================ A: late inputs
@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_late_inputs_are_seen_in_stream_order(streams, case, variant):
    A = streams[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with S.environ(case.env):
        st = case.build()
        if variant == "warmed":
            case.load(st, "decoy")
            case.run(st)
            torch.cuda.synchronize()
        case.load(st, "decoy")
        torch.cuda.synchronize()
        with torch.cuda.stream(A):
            t0 = time.perf_counter()
            e0.record()
            S.hold(A)
            e1.record()
            case.late_copies(st)
            t1 = time.perf_counter()
            case.run(st)
            # (the event behind the hold, not the stream alone: after a wait inside the call the stream is busy again with the
            # call's own last kernels, which says nothing about the hold)
            busy = not A.query() and not e1.query()
            t2 = time.perf_counter()
            got = case.results(st)
        A.synchronize()
        hold_ms, lead_ms = e0.elapsed_time(e1), (t1 - t0) * 1e3
        print(f"{case.name} [{variant}]: hold {hold_ms:.1f} ms, host lead {lead_ms:.3f} ms, call {(t2 - t1) * 1e3:.3f} ms, "
              f"hold in force after the enqueue: {busy}")
        if variant in case.sync:
            assert case.why, "an inspect-class variant names its reason"
            assert hold_ms >= 10.0 * lead_ms, \
                f"the hold ({hold_ms:.1f} ms) was not ten times the host lead ({lead_ms:.3f} ms): the case proved nothing"
        else:
            assert busy, (f"the hold ({hold_ms:.1f} ms) had run out when the call returned: either it was too short -- the case "
                          f"proved nothing -- or this execute-class call waited for the stream")
        with torch.cuda.stream(A):
            case.after(st)
        A.synchronize()
    assert case.violations(host(got), expected(case, "real")) == []


# ======================================================================================= B: plans die behind their last use
OWNERS = [c for c in S.CASES if c.owner]


def run_lifetime(streams, case, destroy):
    """Steps 1 - 7 of part B; `destroy(st)` is what ends the plan's arrays with the handle on B.  Returns (before, probe0, probe1,
    out) as host arrays."""
    A, B = streams[0], streams[1]
    with S.environ(case.env):
        st = case.build()
        case.load(st, "real")
        tiny = Tiny()
        tiny()
        before = [t.clone() for t in st.outs]
        torch.cuda.synchronize()
        with torch.cuda.stream(A):
            S.hold(A)
            case.run(st)
        with torch.cuda.stream(B):
            tiny()
            probe0 = [t.clone() for t in st.outs]
        with torch.cuda.stream(B):
            destroy(st)
            probe1 = [t.clone() for t in st.outs]
        A.synchronize()
        B.synchronize()
        outs = list(st.outs)
    return before, probe0, probe1, outs


def check_lifetime(case, before, probe0, probe1, outs):
    for b, p in zip(before, probe0):
        assert np.array_equal(raw(b), raw(p)), \
            "control: stream B saw the op's output before the destroy -- B was ordered behind A anyway, or the hold had run out"
    want = expected(case, "real")
    assert case.violations(host(before), want) != [], "control: the output held the result before the op ran"
    assert case.violations(host(probe1), want) == [], "what B ran after the destroy was not behind the plan's last use"
    assert case.violations(host(outs), want) == []


@pytest.mark.parametrize("case", OWNERS, ids=repr)
def test_plans_die_behind_their_last_use(streams, case):
    """(The SpMV plan is the regression anchor: spblas_gfx950_plan_destroy did this before the other destroys did.)"""
    check_lifetime(case, *run_lifetime(streams, case, case.drop))


def test_a_new_symbolic_pass_replaces_the_result_behind_the_pending_fill(streams):
    """spgemm_release: a second multiply_compute on the same state, with the handle on B, frees the first result's arrays while
    the fill that reads them is pending on A.  It is inspect-class and synchronises B."""
    case = S.BY_NAME["spgemm_fill_one_shot"]
    g = S.spgemm_operands()
    seen = {}

    def replace(st):
        rp2 = torch.zeros(g.a_shape[0] + 1, dtype=torch.int32, device="cuda")
        c2 = sp.csr_view(None, rp2, None, (g.a_shape[0], g.b_shape[1]), 0)
        sp.multiply_compute(st.info, st.a, st.b, c2)
        seen["rowptr"], seen["nnz"] = rp2, st.info.result_nnz()

    before, probe0, probe1, outs = run_lifetime(streams, case, replace)
    check_lifetime(case, before, probe0, probe1, outs)
    want = expected(case, "real")
    assert seen["nnz"] == want[0].size and np.array_equal(S.to_host(seen["rowptr"]), want[2])


# ================================================================================== C: the probe detects a misordered call
@pytest.mark.parametrize("name", S.MISORDERED)
def test_the_probe_detects_a_misordered_call(streams, name):
    """Correct library code on valid inputs, issued by the test on a stream that is NOT ordered behind the late copies: the
    result is the decoys' -- so a stray launch inside an op would fail part A."""
    case = S.BY_NAME[name]
    A, C = streams[0], streams[2]
    with S.environ(case.env):
        st = case.build()
        case.load(st, "decoy")
        torch.cuda.synchronize()
        behind_hold = torch.cuda.Event()
        with torch.cuda.stream(A):
            S.hold(A)
            behind_hold.record()
            case.late_copies(st)
        with torch.cuda.stream(C):
            case.run(st)
            got = case.results(st)
        C.synchronize()
        held = not behind_hold.query()
        A.synchronize()
        torch.cuda.synchronize()
    assert held, "the hold had run out before the misordered op finished: the case proved nothing"
    got = host(got)
    assert case.violations(got, expected(case, "decoy")) == []
    assert case.violations(got, expected(case, "real")) != []
