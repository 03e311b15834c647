"""Every route of the GEMM launcher (csrc/gemm.hip: launch_gemm / launch_streamk) against the float64 product, on buffers of the
test's own, with the route the call took read back from the launcher's route log (ops.gemm_route_log).

The matrix is helpers.GEMM_CASES: the smallest shapes that reach each of the eleven routes, each in two alignment variants (every
base pointer one float past a 16-byte boundary and odd leading dimensions of A and B in the second), with default routing, with
the options gemm_mid_split / gemm_streamk at 0 (the fallback routes) and inside ops.fixed_order_gemms().  The error of an element is
|got - ref| / (|alpha| sum_k |a_mk b_kn| + |beta c0_mn| + |bias_n|), the maximum is taken over ALL elements and held to
helpers.GEMM_BOUND -- 4 x what the float32 running sum loses at the same case (tests/test_gemm_oracle_cpu.py measures the floors and
proves that every mutation of helpers.GEMM_BUGS lands 10 bounds away or more).  Outputs are NaN where beta = 0, so every element
has to be written (the zero fill of the split routes has to cover strided rows); 4096 canary floats behind the output, one in front
of it in the odd variant, and the padding columns of ldc > N rows have to survive.

MEASURED on the MI355X (pytest -s prints every comparison: route, splitk, tile, worst error as a share of the bound, where it fell).
Every case took the route of the table, in both variants and all four modes; worst error per route as a share of its case's bound
(123 comparisons):
    skinny 48x16                0.12   33x1000x67 NT bias ELU, odd
    m32-split 32x128            0.14   31x130x257 NT alpha 0.5 bias ELU ldc 135
    m32 32x128                  0.29   17x200x300 TN alpha 2 beta 0.5, odd
    mid-split 64x64             0.16   450x200x250 TN beta 1, odd
    streamk-direct 128x128      0.04   130x70x1266 TN
    streamk-lds 128x128         0.08   300x128x1290 NN conv form, odd
    streamk-lds 256x128         0.17   3000x2049x1270 NN, odd
    splitk 128x128 / 64x64      0.09 / 0.10   3072x2048x1280 NN with gemm_streamk = 0 / 1000x40x1100 NN
    half 128x64                 0.34   3072x2048x1280 NN, fixed order
    tile 128x128                0.33   3000x2049x1270 NN, fixed order
    tile 64x64                  0.29   449x193x251 NT bias ReLU ldc 197 with gemm_mid_split = 0
The unsplit routes sit closest to their bounds (one running sum per element, like the floor's); the split routes, whose segments
are shorter sums, at a third of that.  No canary moved and no NaN survived.  Fixed order: bitwise equal on three calls at every case.
Controls on scratch builds, not committed: gemm_tile stopping one k-tile short fails 117 of the 125 tests (the skinny and direct
kernels do not run gemm_tile), the two rows_fill_k launches skipped fails the 13 that run a beta = 0 product on the M <= 32 or mid split.
Kernel instantiations launched: skinny_k<3, true>; gemm_kernel<32, 128, 1, 4> NT / TN; <64, 64, 2, 2> NN / NT / TN; <128, 128, 2, 2>
NN / NT / TN; <128, 64, 2, 2> NN / NT; gemm_streamk_kernel<128, 128, 2, 2> NN / NT / TN and <256, 128, 4, 2> NN;
gemm_tn_direct_kernel<2, 2, 4>; rows_fill_k, rows_bias_act_k, fill_k / fill4_k (NN = <AKC, BKC> true, false; NT true, true; TN false,
false).
"""
import threading

import pytest
import torch

import helpers
from helpers import GEMM_BOUND, GEMM_CANARY, GEMM_CANARY_TAIL, GEMM_CASES, GEMM_VARIANTS
from zeggs import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c["id"] for c in GEMM_CASES]
_INPUTS = {}
MID = [c for c in GEMM_CASES if c["no_mid"] is not None]
STREAMK = [c for c in GEMM_CASES if c["no_streamk"] is not None]
SPLITTING = set(ops.GEMM_SPLITTING_ROUTES)


def _inputs(case, variant):
    """the case's operands on the device, uploaded once"""
    key = (case["id"], variant)
    if key not in _INPUTS:
        d = helpers.gemm_case_data(case, variant)
        _INPUTS[key] = (d["A"].to(DEV), d["B"].to(DEV), None if d["bias"] is None else d["bias"].to(DEV))
    return _INPUTS[key]


def _launch(case, variant):
    """one product through ops.gemm onto a fresh copy of the case's output buffer -> (the whole buffer on the device, route log)"""
    d = helpers.gemm_case_data(case, variant)
    A, B, bias = _inputs(case, variant)
    C = d["C"].to(DEV)
    off = d["off"]
    ops.gemm_route_log(reset=True)
    ops.gemm(A[off:], B[off:], C[off:], case["M"], case["N"], case["K"], d["sa"], d["sb"], (d["ldc"], 1), bias=bias,
             nbatch=case["nbatch"], bs=d["bs"], alpha=case["alpha"], beta=case["beta"], act=case["act"])
    return C, ops.gemm_route_log()


def _took(log):
    return (log["route"], log["splitk"]) + tuple(log["tile"])


def _check(case, variant, C, log, expected, tag):
    """the route log shows `expected` and nothing else; canaries intact; every element within the case's bound"""
    d = helpers.gemm_case_data(case, variant)
    M, N, nb, ldc, off = case["M"], case["N"], case["nbatch"], d["ldc"], d["off"]
    assert _took(log) == tuple(expected), (case["id"], variant, tag, log)
    assert log["counts"] == {expected[0]: 1}, (case["id"], variant, tag, log)
    C = C.cpu()
    body = C[off:off + nb * M * ldc].view(nb, M, ldc)
    assert bool((C[:off] == GEMM_CANARY).all()) and bool((C[off + nb * M * ldc:] == GEMM_CANARY).all()), (case["id"], variant, tag)
    assert C.numel() - (off + nb * M * ldc) == GEMM_CANARY_TAIL
    assert bool((body[:, :, N:] == GEMM_CANARY).all()), (case["id"], variant, tag, "padding columns")
    ref, den = helpers.gemm_truth(case, variant)
    err, where = helpers.gemm_error(body[:, :, :N], ref, den)
    bound = GEMM_BOUND[case["id"]]
    print(f"\nMEASURED {case['id']:36s} {variant:7s} {tag:11s} {log['route']:20s} splitk {log['splitk']:2d} tile {log['tile'][0]}x{log['tile'][1]}: "
          f"worst {err:.3g} = {err / bound:.2f} of the bound, at {where}")
    assert err <= bound, (case["id"], variant, tag, err, bound, where)
    return body[:, :, :N]


class _option:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        ops.set_option(self.name, self.value)

    def __exit__(self, *exc):
        ops.set_option(self.name, 1)
        ops._OPTIONS.pop(self.name, None)
        return False


# ----------------------------------------------------------------------------- 1. the matrix, default routing
@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("case", GEMM_CASES, ids=IDS)
def test_route_and_error(case, variant):
    C, log = _launch(case, variant)
    _check(case, variant, C, log, case["route"], "default")


def test_every_route_is_reached():
    assert {c["route"][0] for c in GEMM_CASES} == set(helpers.GEMM_ROUTES_COVERED)
    assert set(helpers.GEMM_ROUTES_COVERED) | {"none", "streamk-bf16-split", "streamk-dma"} == set(ops.GEMM_ROUTES)


# ----------------------------------------------------------------------------- 2. the option fallbacks
@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("case", MID, ids=helpers.gemm_case_id)
def test_without_the_mid_split(case, variant):
    with _option("gemm_mid_split", 0):
        C, log = _launch(case, variant)
    _check(case, variant, C, log, case["no_mid"], "mid_split=0")


@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("case", STREAMK, ids=helpers.gemm_case_id)
def test_without_stream_k(case, variant):
    with _option("gemm_streamk", 0):
        C, log = _launch(case, variant)
    _check(case, variant, C, log, case["no_streamk"], "streamk=0")


# ----------------------------------------------------------------------------- 3. fixed order
def _fixed_state():
    L = ops.lib()
    prev = L.zeggs_gemm_fixed_order(0)
    L.zeggs_gemm_fixed_order(prev)
    return prev


@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("case", GEMM_CASES, ids=IDS)
def test_fixed_order(case, variant):
    """the route of the table's last column, no counter of a splitting route moves, the bound holds (the beta = 1 cases accumulate
    onto their loaded C), and the bits repeat -- also with another product launched in between"""
    other = GEMM_CASES[5] if case is not GEMM_CASES[5] else GEMM_CASES[10]
    with ops.fixed_order_gemms():
        C, log = _launch(case, variant)
        _check(case, variant, C, log, case["fixed"], "fixed order")
        assert not SPLITTING & set(log["counts"])
        C2, log2 = _launch(case, variant)
        _, olog = _launch(other, "aligned")
        C3, log3 = _launch(case, variant)
        assert olog["route"] == other["fixed"][0] and _took(log2) == _took(log3) == tuple(case["fixed"])
    n = C.numel() - GEMM_CANARY_TAIL
    assert torch.equal(C2[:n].cpu().view(torch.int32), C[:n].cpu().view(torch.int32))        # bitwise, canaries and all
    assert torch.equal(C3[:n].cpu().view(torch.int32), C[:n].cpu().view(torch.int32))


def test_fixed_order_state_is_restored():
    assert _fixed_state() == 0
    with ops.fixed_order_gemms():
        assert _fixed_state() == 1
        with ops.fixed_order_gemms():
            assert _fixed_state() == 1
        assert _fixed_state() == 1              # nested: the inner block puts back what it found
    assert _fixed_state() == 0
    with pytest.raises(ZeroDivisionError):
        with ops.fixed_order_gemms():
            assert _fixed_state() == 1
            1 / 0
    assert _fixed_state() == 0
    case = MID[0]
    _, log = _launch(case, "aligned")
    assert _took(log) == tuple(case["route"])   # ... and the products split again


def test_fixed_order_is_the_calling_threads_alone():
    """a second thread that never entered the block still gets the mid-split route while the first thread is inside it"""
    case = MID[0]
    seen = {}

    def other():
        try:
            seen["state"] = _fixed_state()
            C, log = _launch(case, "aligned")
            torch.cuda.synchronize()
            seen["log"], seen["C"] = log, C
        except Exception as e:                  # noqa: BLE001  (reported by the assertion below)
            seen["error"] = repr(e)
    with ops.fixed_order_gemms():
        ops.gemm_route_log(reset=True)
        t = threading.Thread(target=other)
        t.start()
        t.join()
        mine = ops.gemm_route_log()
        C, log = _launch(case, "aligned")
        assert _took(log) == tuple(case["fixed"])
    assert "error" not in seen, seen
    assert seen["state"] == 0 and _took(seen["log"]) == tuple(case["route"])
    assert mine["route"] == "none" and mine["counts"] == {}        # the log is per thread too
    _check(case, "aligned", seen["C"], seen["log"], case["route"], "2nd thread")
