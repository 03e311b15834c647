"""CPU side of tests/test_gpu_attention.py (the fused attention kernels against a float64 oracle; no GPU needed):
(a) helpers.attention_oracle IS the attention of oracle/nets.py::_mha (identity projections, with and without a mask);
(b) conditioning: what a float32 evaluation of the same oracle loses at every case the GPU file runs -- the floors that
    helpers.ATTN_BOUND is 4 x of -- and that every family is the regime its name says;
(c) negative controls: one wrong line of the kernels, modelled in the oracle (bug=), is at least 10 x the bound on a case the GPU
    file runs, in float64.
The floors themselves: the comment of helpers.ATTN_FLOORS.
"""
import numpy as np
import pytest
import torch

import helpers
from helpers import ATTN_BOUND, attn_bound_key, attn_class

ALL_CASES = helpers.ATTN_SHAPE_CASES + helpers.ATTN_REGIME_CASES + helpers.ATTN_DROPOUT_CASES
_CACHE = {}


def _case(case):
    """(qkv, dO, keep, float64 oracle) of one case of the GPU file; computed once, left unchanged"""
    if case not in _CACHE:
        f, B, NH, L, p = case
        qkv, dO = helpers.attention_case(f, B, NH, L, helpers.attn_case_seed(case))
        keep = helpers.attention_keep(helpers.attn_mask_seed(case), B, NH, L, p) if p > 0 else None
        _CACHE[case] = (qkv, dO, keep, helpers.attention_oracle(qkv, dO, NH, keep))
    return _CACHE[case]


def _wrap_head(bh):
    """one head of the 2^32 case as the GPU file runs it (its inputs there are drawn on the device: another draw of the same
    distribution), masks from the hash restatement"""
    W = helpers.ATTN_WRAP
    qkv, dO = helpers.attention_case("mild", 1, 1, W["L"], W["seed"] + bh)
    keep = helpers.attention_keep(W["seed"], W["B"], W["NH"], W["L"], W["p"], heads=[bh])
    return qkv, dO, keep


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("masked", [False, True])
def test_oracle_is_the_attention_of_the_network_oracle(masked):
    """oracle/nets.py::_mha with projections that compute nothing -- in_proj = [I; a rotation of the channels; their reversal] (q, k
    and v are then three different arrangements of x) plus a bias, out_proj = I -- against attention_oracle on the same q | k | v:
    the output, the gradient carried back to x through the three permutations, and the bias gradient (= dbias), float64, 1e-12."""
    from oracle import nets as onets
    dt = torch.float64
    B, NH, L = 2, 4, 45
    E = 32 * NH
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, L, E, generator=gen, dtype=dt).requires_grad_(True)
    dO = torch.randn(B, L, E, generator=gen, dtype=dt)
    eye = torch.eye(E, dtype=dt)
    in_w = torch.cat([eye, eye.roll(7, dims=0), eye.flip(0)], dim=0)
    in_b = torch.randn(3 * E, generator=gen, dtype=dt).requires_grad_(True)
    keep = helpers.attention_keep(99, B, NH, L, 0.1) if masked else None
    assert keep is None or 0.05 < float((keep == 0).double().mean()) < 0.15
    out = onets._mha(x, in_w, in_b, eye, torch.zeros(E, dtype=dt), nheads=NH, pmask=keep)
    gx, gb = torch.autograd.grad((out * dO).sum(), [x, in_b])
    qkv = torch.nn.functional.linear(x, in_w, in_b).detach()
    O, lse2, dqkv, dsum, dbias = helpers.attention_oracle(qkv, dO, NH, keep)
    assert float((O - out.detach()).abs().max()) <= 1e-12 * float(out.detach().abs().max())
    assert float((dqkv @ in_w - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert float((dbias - gb).abs().max()) <= 1e-12 * float(gb.abs().max())
    # the backward in the kernels' form (D = rowsum(dO . O)) is the same function
    alt = helpers.attention_oracle(qkv, dO, NH, keep, d_from_o=True)
    for a_, b_ in zip(alt, (O, lse2, dqkv, dsum, dbias)):
        assert float((a_ - b_).abs().max()) <= 1e-12 * float(b_.abs().max())
    # the by-products, from their definitions
    q = qkv[..., :E].reshape(B, L, NH, 32).transpose(1, 2)
    k = qkv[..., E:2 * E].reshape(B, L, NH, 32).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / np.sqrt(32.0)
    ref_lse2 = torch.log2(torch.exp(s - s.amax(-1, keepdim=True)).sum(-1)) + s.amax(-1) * helpers.LOG2E
    assert float((lse2 - ref_lse2.reshape(B * NH, L)).abs().max()) <= 1e-12 * float(ref_lse2.abs().max())
    ref_dsum = (dO * O).reshape(B, L, NH, 32).sum(-1).transpose(1, 2).reshape(B * NH, L)
    assert float((dsum - ref_dsum).abs().max()) <= 1e-12 * float(ref_dsum.abs().max())


# ------------------------------------------------------------------ (b)
def test_families_are_the_regimes_they_are_named_for():
    for case in ALL_CASES:
        f, B, NH, L, p = case
        qkv, dO, keep, ref = _case(case)
        E = 32 * NH
        q = qkv.double()[..., :E].reshape(B, L, NH, 32).transpose(1, 2)
        k = qkv.double()[..., E:2 * E].reshape(B, L, NH, 32).transpose(1, 2)
        s = q @ k.transpose(-1, -2) / np.sqrt(32.0)
        P = torch.softmax(s, -1)
        if f == "mild" and L >= 31:
            assert 0.8 < float(s.std()) < 1.2, (case, float(s.std()))
        if f in ("g3", "g6"):
            assert abs(float(s.std()) / (9.0 if f == "g3" else 36.0) - 1) < 0.2 and float(P.max()) > 0.999, case
        if f == "lastkey" and L >= 33:
            assert float((s.argmax(-1) == L - 1).double().mean()) > 0.95, case
        if f == "onehot" and L >= 2:
            assert float(P[..., 0].min()) > 0.999 and float((P[..., 0].float() == 1.0).double().mean()) > 0.95, case      # one-hot in float32
        if f == "offset":
            assert float(s.mean()) > 60.0, case
        if f == "equal":
            assert float((P - 1.0 / L).abs().max()) < 1e-15, case
        if keep is not None:
            assert 0.08 < float((keep == 0).double().mean()) < 0.12, case


def _merge(worst, cls, errs):
    for t, e in errs.items():
        k = attn_bound_key(t)
        worst[cls][k] = max(worst[cls].get(k, 0.0), e)


def test_float32_floors_are_within_a_quarter_of_the_bounds():
    """Every case of the GPU file: attention_oracle in float32, its backward in the kernels' form (d_from_o=True: D = rowsum(dO . O)
    from the output), against float64 on the same float32 inputs, per tensor, in the measure of attention_errors.  The largest per class is the floor; ATTN_BOUND = 4 x ATTN_FLOORS and every measured floor must be
    <= its recorded one (i.e. <= bound / 4) -- and not far below it, so that the constants stay what this test measures."""
    worst = {c: {} for c in ATTN_BOUND}
    for case in ALL_CASES:
        f, B, NH, L, p = case
        qkv, dO, keep, ref = _case(case)
        errs = helpers.attention_errors(helpers.attention_oracle(qkv, dO, NH, keep, dtype=torch.float32, d_from_o=True), ref)
        assert all(np.isfinite(e) for e in errs.values()), (case, errs)
        _merge(worst, attn_class(f, L), errs)
    for bh in (0, 268):         # the 2^32 case: L = 4000 (heads 267 and 269 are two more draws of the same thing)
        qkv, dO, keep = _wrap_head(bh)
        ref = helpers.attention_oracle(qkv, dO, 1, keep)
        errs = helpers.attention_errors(helpers.attention_oracle(qkv, dO, 1, keep, dtype=torch.float32, d_from_o=True), ref)
        print(f"\nwrap head {bh}: " + " ".join(f"{t} {e:.2e}" for t, e in errs.items()))
        _merge(worst, "mild", errs)
    for c, w in worst.items():
        print(f"\n{c:8s} " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    for c, w in worst.items():
        for k, v in w.items():
            assert v <= ATTN_BOUND[c][k] / 4.0, (c, k, v, ATTN_BOUND[c][k])
            assert v >= ATTN_BOUND[c][k] / 4.0 / 1.5, (c, k, v, "the recorded floor is stale")


# ------------------------------------------------------------------ (c)
def _worst_ratio(bug, cases):
    """largest error / bound over the tensors and `cases` of the float64 oracle with `bug` against the float64 oracle without"""
    best = (0.0, None, None)
    for case in cases:
        f, B, NH, L, p = case
        qkv, dO, keep, ref = _case(case)
        errs = helpers.attention_errors(helpers.attention_oracle(qkv, dO, NH, keep, bug=bug), ref)
        for t, e in errs.items():
            r = e / ATTN_BOUND[attn_class(f, L)][attn_bound_key(t)]
            if r > best[0]:
                best = (r, case, t)
    return best


NODROP = helpers.ATTN_SHAPE_CASES + helpers.ATTN_REGIME_CASES
CONTROLS = [("O_row", NODROP), ("dQ_row", NODROP), ("dK_row", NODROP), ("dV_row", NODROP), ("key_L", ALL_CASES),
            ("mask_transposed", helpers.ATTN_DROPOUT_CASES), ("bwd_mask_redrawn", helpers.ATTN_DROPOUT_CASES),
            ("dsum_undropped", helpers.ATTN_DROPOUT_CASES), ("lse_natural", NODROP), ("dK_without_ln2", NODROP)]


@pytest.mark.parametrize("bug,cases", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_negative_control_is_ten_times_the_bound(bug, cases):
    ratio, case, tensor = _worst_ratio(bug, cases)
    print(f"\n{bug}: {ratio:.1f} x the bound in {tensor} of {helpers.attn_case_id(case)}")
    assert ratio >= 10.0, (bug, ratio, case, tensor)


def test_row_controls_at_the_lengths_the_encoder_tests_run():
    """a 1e-3 error in ONE row of one head of O / dQ / dK / dV -- a tenth of what the encoder-level tests let pass -- is >= 10 x the
    bound at (2, 4, 129) and (2, 4, 257), family mild"""
    for L in (129, 257):
        for bug in ("O_row", "dQ_row", "dK_row", "dV_row"):
            ratio, case, tensor = _worst_ratio(bug, [("mild", 2, 4, L, 0.0)])
            print(f"\nL = {L} {bug}: {ratio:.1f} x the bound in {tensor}")
            assert ratio >= 10.0, (L, bug, ratio)


def test_negative_control_hash_high_word_ignored():
    """the 2^32 case: head 269 lies wholly beyond element 2^32; a mask hashed without the high index word moves O by > 10 x the bound.
    Heads below 2^32 are untouched by the bug, and inside head 268 the masks part exactly at row 1741, key 3296."""
    W = helpers.ATTN_WRAP
    L, p, seed = W["L"], W["p"], W["seed"]
    first = 2 ** 32 - 268 * L * L
    assert (first // L, first % L) == (1741, 3296)
    a, b = (helpers.hash_keep_scale(seed, 268 * L * L, L * L, p, bug=g) for g in (None, "hi_ignored"))
    assert np.array_equal(a[:first], b[:first]) and 0.15 < float((a[first:] != b[first:]).mean()) < 0.21     # 2 p (1 - p) = 0.18
    assert np.array_equal(helpers.hash_keep_scale(seed, 267 * L * L, 4096, p), helpers.hash_keep_scale(seed, 267 * L * L, 4096, p, bug="hi_ignored"))
    qkv, dO, keep = _wrap_head(269)
    bad = helpers.attention_keep(seed, W["B"], W["NH"], L, p, heads=[269], bug="hi_ignored")
    with torch.no_grad():
        E = 32
        q, k, v = (qkv.double()[0, :, i * E:(i + 1) * E] for i in range(3))
        P = torch.softmax(q @ k.T / np.sqrt(32.0), -1)
        O, Ob = (P * keep[0, 0]) @ v, (P * bad[0, 0]) @ v
    e = helpers.relerr(Ob, O)
    print(f"\nhigh word ignored: O moves by {e:.2e} = {e / ATTN_BOUND['mild']['O']:.0f} x the bound")
    assert e >= 10.0 * ATTN_BOUND["mild"]["O"]


def test_hash_restatement_basics():
    """the NumPy restatement of the mask hash: keep rate, determinism, dependence on both seed words and on the high index word
    (bit-equality with the device: tests/test_gpu_attention.py)"""
    m = helpers.hash_keep_scale(5, 0, 1 << 16, 0.1)
    assert set(np.unique(m)) == {0.0, 1.0 / (1.0 - 0.1)}
    assert abs(float((m == 0).mean()) - 0.1) < 0.01
    assert not np.array_equal(m, helpers.hash_keep_scale(5 + (1 << 32), 0, 1 << 16, 0.1))
    assert not np.array_equal(m, helpers.hash_keep_scale(6, 0, 1 << 16, 0.1))
    assert not np.array_equal(m, helpers.hash_keep_scale(5, 1 << 32, 1 << 16, 0.1))
    assert np.array_equal(m[100:200], helpers.hash_keep_scale(5, 100, 100, 0.1))
