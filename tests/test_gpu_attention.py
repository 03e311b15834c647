"""The fused attention kernels of the style encoder (csrc/attention.hip: softmax(QK^T) -> dropout -> .V in one launch, backward
recomputed from the row log-sum-exp) against the GEMM + softmax + GEMM path they replace, through the whole StyleEncoder
forward + backward: sequence lengths that are / are not multiples of the 32-key and 128-query tiles, dropout masks on (the
same counter-hash masks on both paths) and off.  Parity with the reference itself: tests/test_gpu_parity.py and
tests/test_gpu_full_shapes.py run on the fused path (the default).

THE KERNELS THEMSELVES (below the encoder-level test): zeggs_test_attention_fwd / _bwd -- k_attn_fwd / k_attn_bwd on the test's own
buffers -- against helpers.attention_oracle in float64, per tensor, within helpers.ATTN_BOUND (4 x what a float32 evaluation of the
same oracle loses; tests/test_attention_oracle_cpu.py measures the floors and proves the comparison sharp).  The forward compares
O and the base-2 log-sum-exp; the backward is fed the kernel's own O and lse and compares dQ, dK, dV, rowsum(dO . O) and the bias
gradient.  Every call pre-fills its outputs with NaN (every element must be written) and allocates them with a canary tail of 4 096
floats (no clamped row or key may store).  Template instantiations launched:
    shapes, regimes (p = 0)      attn_fwd_k<DROP=false>;  one_launch = 1: attn_bwd_k<false> (dQ body + dK/dV body <false, OWN=true>);
                                 one_launch = 0: attn_bwd_q_k<false> + attn_bwd_kv_k<false> (dK/dV body <false, OWN=false>)
    dropout, 2^32 (p = 0.1)      attn_fwd_k<true>;  attn_bwd_k<true> (<true, OWN=true>);  attn_bwd_q_k<true> + attn_bwd_kv_k<true> (<true, false>)
    dbias                        both backward forms at p = 0 and p = 0.1, dbias null and pre-loaded
    refusals                     nothing
Measured on the MI355X (worst error, as a share of its bound, and where; one_launch 1 and 0 agree to the last digit shown except
for the float atomics of dbias):
    shapes + regimes   O 6.8e-6 (0.26, offset L = 257)   lse2 1.4e-7 (0.27, equal 257)   dQ 7.2e-5 (0.28, lastkey L = 2, class cancel)
                       dK 8.2e-6 (0.27, g6 257)   dV 5.2e-6 (0.17, g6 257)   dsum 9.7e-8 (0.35, lastkey L = 2)   dbias 6.7e-6 (0.40, offset 257)
                       family mild alone: every tensor <= 1.0e-6, <= 0.24 of its bound (dbias at E = 32: 0.37); `equal`: dQ 1.9e-6 (0.18)
    dropout            O 7.2e-7 (0.16)   lse2 1.1e-7 (0.21)   dQ 3.1e-6 (0.09, g3 257)   dK 1.2e-6 (0.12)   dV 8.0e-7 (0.08)   dbias 6.3e-7 (0.23);
                       lastkey: the mask drops the arg-max key of 19 / 116 / 225 rows; without the mask 7 000 ... 100 000 x the bound
    dbias              pre-loaded: 1.1e-6 (0.41)
    2^32               heads 0, 267, 268, 269: O 2.0e-6 (0.44)   lse2 1.4e-7 (0.25)   dQ 3.3e-6 (0.32)   dK 2.0e-6 (0.19)   dV 4.2e-6 (0.40)
                       dsum 1.6e-6 (0.49); 1.7 s, of which 0.06 s on the device -- forward and BOTH backward forms kept
No kernel was found wrong.  One excess on the first run: `lastkey` at L = 2, dQ 7.2e-5 and dbias 8.2e-5 against float32 floors of
2.1e-5 / 9.3e-6 -- the kernels take D = rowsum(dO . O) from the stored output, autograd's softmax backward takes sum_k P_k dP_k and its
roundings cancel against the minuend; the float32 restatement now runs the kernels' form (attention_oracle(d_from_o=True)), its floor
there is 6.2e-5 / 5.5e-5, and that one case has a class of its own (helpers.attn_class) so that the peaked bounds stay where they were.
Wall time: the 62 new tests 4.7 s together, each <= 0.1 s but the 2^32 case (1.7 s)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import helpers
from zeggs import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(st, x, eps, w, fused, dropout):
    ops.set_option("fused_attention", fused)
    ops.manual_seed(77)
    st.train() if dropout else st.eval()
    st.zero_grad()
    z, mu, lv = st(x, 1.0, eps=eps)
    (z * w[0] + mu * w[1] + lv * w[2]).sum().backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (z, mu, lv)], {k: p.grad.detach().clone() for k, p in st.named_parameters()}


@pytest.mark.parametrize("one_launch", [1, 0])
@pytest.mark.parametrize("L,dropout", [(384, True), (77, True), (200, False), (33, False), (512, True)])
def test_fused_attention_matches_the_gemm_softmax_path(L, dropout, one_launch):
    """one_launch = 1 (default since round 6): the dQ and the dK / dV pass as ONE grid (blockIdx.z = pass; the dK / dV workgroups
    form rowsum(dO . O) themselves); 0: two launches, the second reading what the first stored."""
    ops.set_option("attn_bwd_one_launch", one_launch)
    _, _, st = helpers.build_nets()
    st = st.to(DEV)
    g = torch.Generator().manual_seed(L)
    B = 3
    x = torch.randn(B, L, synth.POSE_IN, generator=g).to(DEV)
    eps = torch.randn(B, 64, generator=g).to(DEV)
    w = [torch.randn(B, 64, generator=g).to(DEV) for _ in range(3)]
    try:
        out1, g1 = _run(st, x, eps, w, 1, dropout)
        out0, g0 = _run(st, x, eps, w, 0, dropout)
    finally:
        ops.set_option("fused_attention", 1)
        ops.set_option("attn_bwd_one_launch", 1)
    for a, b in zip(out1, out0):
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    worst = 0.0
    for k in g0:
        scale = max(1e-12, float(g0[k].abs().max()))
        e = float((g1[k] - g0[k]).abs().max()) / scale
        worst = max(worst, e)
        assert e < 2e-4, (k, e)
    print(f"\nL={L} dropout={dropout}: fused vs unfused worst gradient difference {worst:.2e} of the tensor's max")


# ----------------------------------------------------------------------------- the kernels against the float64 oracle
TAIL, CANARY = 4096, 12345.0


def _buf(shape, fill):
    """a device float32 array of `shape`, filled with `fill`, in front of a tail of TAIL canary floats -> (view, whole allocation)"""
    n = int(np.prod(shape))
    whole = torch.full((n + TAIL,), CANARY, device=DEV, dtype=torch.float32)
    whole[:n] = fill
    return whole[:n].view(*shape), whole


def _dev(t):
    """a read-only input on the device, canary tail behind it as well"""
    v, whole = _buf(tuple(t.shape), 0.0)
    v.copy_(t)
    return v, whole


def _untouched(whole, what):
    assert bool((whole[-TAIL:] == CANARY).all()), f"{what}: the canary tail behind the buffer was written"


def _fwd_raw(qkv, O, lse, B, L, E, NH, p, seed):
    return ops.lib().zeggs_test_attention_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(O.data_ptr()), C.c_void_p(lse.data_ptr()), B, L,
                                              E, NH, C.c_float(p), C.c_uint64(int(seed)), ops._stream())


def _bwd_raw(qkv, O, lse, dO, dqkv, dsum, dbias, B, L, E, NH, p, seed):
    return ops.lib().zeggs_test_attention_bwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(O.data_ptr()), C.c_void_p(lse.data_ptr()),
                                              C.c_void_p(dO.data_ptr()), C.c_void_p(dqkv.data_ptr()), C.c_void_p(dsum.data_ptr()),
                                              C.c_void_p(dbias.data_ptr()) if dbias is not None else None, B, L, E, NH, C.c_float(p),
                                              C.c_uint64(int(seed)), ops._stream())


def _last_error():
    return ops.lib().zeggs_last_error().decode()


def attn_forward(qkv_d, B, L, NH, p, seed):
    """-> (O [B, L, E], lse [B NH, L]) on the device: written everywhere, nothing written behind them"""
    E = 32 * NH
    (O, Ow), (lse, lw) = _buf((B, L, E), float("nan")), _buf((B * NH, L), float("nan"))
    assert _fwd_raw(qkv_d, O, lse, B, L, E, NH, p, seed) == 0, _last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(O).all()) and bool(torch.isfinite(lse).all()), "forward: an element of O / lse was not written"
    _untouched(Ow, "O"), _untouched(lw, "lse")
    return O, lse


def attn_backward(qkv_d, O, lse, dO_d, B, L, NH, p, seed, one_launch, dbias=None):
    """-> (dqkv, dsum, dbias) on the device under attn_bwd_one_launch = one_launch (restored); dbias: None, or the pre-load"""
    E = 32 * NH
    (dqkv, qw), (dsum, sw) = _buf((B, L, 3 * E), float("nan")), _buf((B * NH, L), float("nan"))
    db, bw = (None, None) if dbias is None else _dev(dbias)
    ops.set_option("attn_bwd_one_launch", one_launch)
    try:
        rc = _bwd_raw(qkv_d, O, lse, dO_d, dqkv, dsum, db, B, L, E, NH, p, seed)
        torch.cuda.synchronize()
    finally:
        ops.set_option("attn_bwd_one_launch", 1)
    assert rc == 0, _last_error()
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dsum).all()), "backward: an element of dqkv / dsum was not written"
    _untouched(qw, "dqkv"), _untouched(sw, "dsum")
    if db is not None:
        _untouched(bw, "dbias")
    return dqkv, dsum, db


def _fmt(errs, bound):
    return "  ".join(f"{k} {e:.1e} ({e / bound[helpers.attn_bound_key(k)]:.2f})" for k, e in errs.items())


def _run_case(case, keep):
    """forward + both backward forms of one case against the float64 oracle -> (inputs on the device, O, lse, oracle, errors)"""
    f, B, NH, L, p = case
    qkv, dO = helpers.attention_case(f, B, NH, L, helpers.attn_case_seed(case))
    seed = helpers.attn_mask_seed(case)
    ref = helpers.attention_oracle(qkv, dO, NH, keep)
    (qkv_d, _), (dO_d, _) = _dev(qkv), _dev(dO)
    O, lse = attn_forward(qkv_d, B, L, NH, p, seed)
    cls = helpers.attn_class(f, L)
    bound = helpers.ATTN_BOUND[cls]
    errs = helpers.attention_errors((O, lse, None, None, None), ref)
    print(f"\n{helpers.attn_case_id(case)} forward: {_fmt(errs, bound)}   [error (share of the bound)]")
    helpers.assert_attention(errs, cls, "forward")
    zero = torch.zeros(3 * 32 * NH)
    for one_launch in (1, 0):
        dqkv, dsum, db = attn_backward(qkv_d, O, lse, dO_d, B, L, NH, p, seed, one_launch, dbias=zero)
        errs = helpers.attention_errors((None, None, dqkv, dsum, db), ref)
        print(f"{helpers.attn_case_id(case)} backward one_launch={one_launch}: {_fmt(errs, bound)}")
        helpers.assert_attention(errs, cls, f"backward one_launch={one_launch}")
    return qkv_d, dO_d, O, lse, ref


@pytest.mark.parametrize("case", helpers.ATTN_SHAPE_CASES, ids=helpers.attn_case_id)
def test_kernels_vs_oracle_shapes(case):
    """family mild, p = 0: lengths either side of the 32-key tile and the 128-query workgroup (L = 129: a workgroup with one live
    row and 127 clamped ones), L = 1 and 2, E = 32, 64, 128 and 256"""
    _run_case(case, None)


@pytest.mark.parametrize("case", helpers.ATTN_REGIME_CASES, ids=helpers.attn_case_id)
def test_kernels_vs_oracle_regimes(case):
    """p = 0: peaked and one-hot rows, the row maximum in the last (partial) key tile, a common logit offset, all-equal keys"""
    _run_case(case, None)


@pytest.mark.parametrize("case", helpers.ATTN_DROPOUT_CASES, ids=helpers.attn_case_id)
def test_kernels_vs_oracle_dropout(case):
    """p = 0.1 with the device's own masks read back (zeggs_dropout on ones, the seed passed straight to the entries).  The hash
    restatement gives the same masks; `lastkey`: the mask drops some row's arg-max key; without the mask the comparison fails by
    more than 100 x the bound."""
    f, B, NH, L, p = case
    seed = helpers.attn_mask_seed(case)
    keep = helpers._device_keep_scale((B, NH, L, L), p, seed)
    mine = helpers.attention_keep(seed, B, NH, L, p)
    assert torch.equal(keep, mine), f"the NumPy restatement of the mask hash differs from the device in {int((keep != mine).sum())} elements"
    qkv_d, dO_d, O, lse, ref = _run_case(case, keep)
    qkv, dO = helpers.attention_case(f, B, NH, L, helpers.attn_case_seed(case))
    if f == "lastkey":
        E = 32 * NH
        q = qkv.double()[..., :E].reshape(B, L, NH, 32).transpose(1, 2)
        k = qkv.double()[..., E:2 * E].reshape(B, L, NH, 32).transpose(1, 2)
        amax = (q @ k.transpose(-1, -2)).argmax(-1, keepdim=True)
        dropped = int((keep.gather(-1, amax) == 0).sum())
        print(f"lastkey: the mask drops the arg-max key of {dropped} of {B * NH * L} rows")
        assert dropped >= 1
    cls = helpers.attn_class(f, L)
    bound = helpers.ATTN_BOUND[cls]
    dqkv, dsum, db = attn_backward(qkv_d, O, lse, dO_d, B, L, NH, p, seed, 1, dbias=torch.zeros(3 * 32 * NH))
    blind = helpers.attention_errors((O, None, dqkv, None, None), helpers.attention_oracle(qkv, dO, NH, None))
    print(f"against the oracle WITHOUT the mask: {_fmt(blind, bound)}")
    for k, e in blind.items():
        assert e > 100.0 * bound[helpers.attn_bound_key(k)], (k, e)


@pytest.mark.parametrize("p", [0.0, helpers.ATTN_P])
@pytest.mark.parametrize("one_launch", [1, 0])
def test_bias_gradient_null_and_preloaded(one_launch, p):
    """dbias = null: the call runs and gives the same dqkv bit for bit; dbias pre-loaded with randn: the result is the pre-load plus
    the float64 column sums of dqkv (the kernels add with atomics, they do not initialise)"""
    case = ("mild", 3, 2, 129, p)
    f, B, NH, L, _ = case
    qkv, dO = helpers.attention_case(f, B, NH, L, helpers.attn_case_seed(case))
    seed = helpers.attn_mask_seed(case)
    keep = helpers._device_keep_scale((B, NH, L, L), p, seed) if p > 0 else None
    ref = helpers.attention_oracle(qkv, dO, NH, keep)
    (qkv_d, _), (dO_d, _) = _dev(qkv), _dev(dO)
    O, lse = attn_forward(qkv_d, B, L, NH, p, seed)
    pre = torch.randn(3 * 32 * NH, generator=torch.Generator().manual_seed(3))
    dq0, ds0, none = attn_backward(qkv_d, O, lse, dO_d, B, L, NH, p, seed, one_launch, dbias=None)
    dq1, ds1, db = attn_backward(qkv_d, O, lse, dO_d, B, L, NH, p, seed, one_launch, dbias=pre)
    assert none is None and torch.equal(dq0, dq1) and torch.equal(ds0, ds1)
    want = pre.double() + ref[4]
    errs = helpers.attention_errors((None, None, dq1, ds1, db), ref[:4] + (want,))
    bound = helpers.ATTN_BOUND["mild"]
    print(f"\none_launch={one_launch} p={p}: {_fmt(errs, bound)}")
    helpers.assert_attention(errs, "mild")
    assert helpers.relerr(db.cpu().double() - pre.double(), ref[4]) < 4 * bound["dbias"]      # (the pre-load's own float32 rounding)


def test_entries_refuse_and_launch_nothing():
    """E / NH != 32, L = 0, p = 1, a pointer offset by one float: non-zero with its message, and no output element is touched.  The
    shape decides, not the fused_attention option: with the option off a supported shape still runs."""
    B, NH, L = 2, 4, 33
    E = 32 * NH
    qkv, dO = helpers.attention_case("mild", B, NH, L, 1)
    (qkv_d, _), (dO_d, _) = _dev(qkv), _dev(dO)
    O, lse = attn_forward(qkv_d, B, L, NH, 0.0, 0)
    outs = [_buf((B * L * 3 * E + 4,), float("nan"))[0] for _ in range(4)]      # O, lse, dqkv, dsum stand-ins, room for the offset
    db = torch.full((3 * E + 4,), float("nan"), device=DEV)
    off = lambda t: t[1:]  # noqa: E731
    fwd_bad = [((qkv_d, outs[0], outs[1], B, L, E + 4, NH, 0.0, 0), "head width"), ((qkv_d, outs[0], outs[1], B, L, 64, 4, 0.0, 0), "head width"),
               ((qkv_d, outs[0], outs[1], B, 0, E, NH, 0.0, 0), ">= 1"), ((qkv_d, outs[0], outs[1], 0, L, E, NH, 0.0, 0), ">= 1"),
               ((qkv_d, outs[0], outs[1], B, L, E, NH, 1.0, 0), "p < 1"), ((qkv_d, outs[0], outs[1], B, L, E, NH, -0.1, 0), "p < 1"),
               ((off(qkv_d.flatten()), outs[0], outs[1], B, L - 1, E, NH, 0.0, 0), "aligned"),
               ((qkv_d, off(outs[0]), outs[1], B, L, E, NH, 0.0, 0), "aligned"), ((qkv_d, outs[0], off(outs[1]), B, L, E, NH, 0.0, 0), "aligned")]
    for args, msg in fwd_bad:
        assert _fwd_raw(*args) != 0 and msg in _last_error(), (args[3:], _last_error())
    good = (qkv_d, O, lse, dO_d, outs[2], outs[3], db)
    bwd_bad = [(good, (B, L, E, 3, 0.0, 0), "head width"), (good, (B, 0, E, NH, 0.0, 0), ">= 1"), (good, (B, L, E, NH, 1.0, 0), "p < 1")]
    for i in range(7):
        ptrs = list(good)
        ptrs[i] = off(ptrs[i].flatten())
        bwd_bad.append((tuple(ptrs), (B, L, E, NH, 0.0, 0), "aligned"))
    for ptrs, rest, msg in bwd_bad:
        assert _bwd_raw(*ptrs, *rest) != 0 and msg in _last_error(), (rest, _last_error())
    torch.cuda.synchronize()
    for t in outs + [db]:
        assert bool(torch.isnan(t).all()), "a refused call wrote to its outputs"
    ops.set_option("fused_attention", 0)
    try:
        O2, lse2 = attn_forward(qkv_d, B, L, NH, 0.0, 0)
    finally:
        ops.set_option("fused_attention", 1)
    assert torch.equal(O2, O) and torch.equal(lse2, lse)


@pytest.mark.parametrize("seed", [1, 0xDEADBEEF12345678, 2 ** 63 + 77])
def test_hash_restatement_is_the_device_hash(seed):
    """helpers.hash_keep_scale (csrc/common.h's mix32 / hash_key / mix32k restated in NumPy) == zeggs_dropout read back, bit for bit
    over the first 2^20 element indices: what the 2^32 case takes its masks from"""
    n = 1 << 20
    dev = helpers._device_keep_scale((n,), helpers.ATTN_P, seed).numpy()
    mine = helpers.hash_keep_scale(seed, 0, n, helpers.ATTN_P)
    assert np.array_equal(dev == 0, mine == 0), f"{int(((dev == 0) != (mine == 0)).sum())} of {n} mask bits differ"
    assert np.array_equal(dev, mine)


def test_element_index_crosses_2_to_the_32():
    """(B, NH, E, L) = (270, 1, 32, 4000), p = 0.1: element 2^32 of the [B NH, L, L] probabilities lies in head 268 at row 1741, key
    3296 -- the carry from the low into the high index word happens inside a row (prow64, phi + (lo < prow), the koff form of the
    dK / dV pass).  Heads are independent: the oracle runs for heads 0, 267, 268 and 269, masks from the hash restatement (pinned
    to the device above).  Class mild.  Inputs are drawn on the device (1.2 GB)."""
    W = helpers.ATTN_WRAP
    B, NH, L, p, seed = W["B"], W["NH"], W["L"], W["p"], W["seed"]
    assert (268 * L * L < 2 ** 32 < 269 * L * L) and divmod(2 ** 32 - 268 * L * L, L) == (1741, 3296)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(seed)
    qkv_d = torch.randn(B, L, 96, device=DEV, generator=gen)
    dO_d = torch.randn(B, L, 32, device=DEV, generator=gen)
    O = torch.full((B, L, 32), float("nan"), device=DEV)
    lse = torch.full((B, L), float("nan"), device=DEV)
    assert _fwd_raw(qkv_d, O, lse, B, L, 32, NH, p, seed) == 0, _last_error()
    dq = {}
    for one_launch in (1, 0):
        dqkv = torch.full((B, L, 96), float("nan"), device=DEV)
        dsum = torch.full((B, L), float("nan"), device=DEV)
        ops.set_option("attn_bwd_one_launch", one_launch)
        try:
            rc = _bwd_raw(qkv_d, O, lse, dO_d, dqkv, dsum, None, B, L, 32, NH, p, seed)
            torch.cuda.synchronize()
        finally:
            ops.set_option("attn_bwd_one_launch", 1)
        assert rc == 0, _last_error()
        assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dsum).all())
        dq[one_launch] = (dqkv[list(W["heads"])].cpu(), dsum[list(W["heads"])].cpu())
        del dqkv, dsum
    assert bool(torch.isfinite(O).all()) and bool(torch.isfinite(lse).all())
    t1 = time.perf_counter()
    bound = helpers.ATTN_BOUND["mild"]
    for i, bh in enumerate(W["heads"]):
        keep = helpers.attention_keep(seed, B, NH, L, p, heads=[bh])
        ref = helpers.attention_oracle(qkv_d[bh:bh + 1].cpu(), dO_d[bh:bh + 1].cpu(), 1, keep)
        for one_launch in (1, 0):
            got = (O[bh:bh + 1], lse[bh:bh + 1], dq[one_launch][0][i:i + 1], dq[one_launch][1][i:i + 1], None)
            errs = helpers.attention_errors(got, ref)
            print(f"\nhead {bh} one_launch={one_launch}: {_fmt(errs, bound)}")
            helpers.assert_attention(errs, "mild", f"head {bh} one_launch={one_launch}")
    print(f"\ndevice part {t1 - t0:.2f} s, oracle part {time.perf_counter() - t1:.2f} s")
