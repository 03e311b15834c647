"""The animation kernels either side of the decoder (csrc/anim.hip, csrc/anim_math.h) at other rigs, frame counts and rotations than
the one skeleton of tests/test_gpu_parity.py (75 joints, Hips = joint 0, dt = 1/60, N = 4 / 5 / 24 / 257 / 1000, smooth rotations).

The device is always compared with the float64 oracle (oracle/anim.py, pinned to the reference by tests/test_oracle_golden.py), never
kernel against kernel.  tests/test_anim_oracle_cpu.py proves on the CPU that every case below meets the conditions it was built for
and that ten plausible kernel mistakes are >= 10x these bounds away.  No bound is new:
  the fourteen float64 feature arrays 1e-9, ltxy / ctxy (float32) 1e-6      test_anim_features_vs_oracle_and_reference
  BVH positions 1e-9                                                       test_pose_to_bvh_vs_oracle_and_reference
each per array with atol = rtol (helpers.anim_errors: |got - ref| / (1 + |ref|)).  Euler angles are compared as rotations, || q_dev -
s q_ora ||_inf <= 1e-9 after sign alignment (the DIFFERENCE: |dot| - 1 is quadratic in the error and hides it), through the exact
inverse of each to_euler (helpers.BVH_EULER_INVERSE: the reference's "xzy" formula inverts Ry Rz Rx, not from_euler("xzy")), and where
the oracle's asin angle is below 89 degrees also angle by angle at 1e-9 degrees.

Features (zeggs_anim_features; helpers.ANIM_CASES, clips of helpers.anim_clip; all 16 arrays in full):
  rigs      j3 (the smallest the wrapper takes), j24-root (Hips below a Root joint: global_of walks up from it, joint 0 is not Hips),
            j64 / j65 (anim_unroll_k: one full block of 64 joints / one joint in a second block), j130 (Head 44 levels deep, three
            blocks), j1 (Hips = Spine2 = Head = 0: raw ABI only), each at N = 10
  frames    j3 and j24-root at N = 4, 5, 8, 9, 10, 17, 64, 65: the unroll's groups of eight from frame 1 and its scalar tail (N = 8: tail
            only, 9: one group, no tail, 10: a tail of one, 17: two groups), the 64-frame blocks of anim_root_k / anim_char_k (64, 65);
            j65 and j130 at N = 17
  flips     every clip has a joint whose raw quaternion flips against the frame before in EVERY frame (s_i = (s_{i-1} d_i < 0)
            alternates; d_i < 0 alone gives -1 throughout), others whose channel runs through the wrap every few frames
  median    gaze columns x and z change sign (the order of dkey across the sign bit) with the middle order statistics > 1e-3 apart,
            column y is N times 0.0; static_head (N = 9, 10): all N candidates are the same three doubles
  static    Spine2 keeps its angles: lvrt must be EXACTLY zero there (dq_to_helical at n = 0), as the reference's is
  orders    zyx, xyz, yzx, xzy on j24-root; dt = 1/30 and 1/120 on j3
BVH conversion (zeggs_pose_to_bvh through anim.bvh_channels; helpers.bvh_case): J = 1, 3, 65 x T = 1, 2, 300 (J = 65, T = 300: 77 blocks
of 256 threads), both orders, no start / identity start / general start; two-axis rows scaled by 0.3 ... 3 each and sheared by 0.3,
from rotations chosen per branch of dq_from_xy (trace; half turns +-30 degrees about axes near x, y, z, a quarter of them exact half
turns); the bound is asserted per branch the oracle takes, and that branch must have items wherever the case has 32 or more.
Near-pole rows (asin angle +-(90 - 10^-k) degrees, k = 1, 2, 3) at the same bound; exact-pole rows (helpers.bvh_pole_case: float32 is
what the ABI takes, so |sin| > 1 comes from a root quaternion one float32 ulp above unit norm) only finite and within 1e-3 degrees
of +-90: the reference's formula is undetermined there.
Table form (zeggs_pose_to_bvh_table through capi): seq reversed (joint 0 last, every joint moved), both orders, the whole clip with
ref = NULL, chunks [0, 7), [7, 8), [8, 20) with the clip's frame 0 as reference; expected: the oracle's bvh_channels of the WHOLE clip.
Every destination of the raw-ABI tests is a view into a larger buffer of sentinels that must be intact either side afterwards.
Not covered: the grid-stride loops beyond 8192 blocks (more than 700 k frames).

Order codes through the raw ABI: zeggs_pose_to_bvh(_table) return -1 for anything but 0 / zyx (6) / xzy (24) -- 27 and 33 (yxz) used
to write zyx angles silently -- and zeggs_anim_features for a code whose three 2-bit axes are no permutation of {0, 1, 2} (an axis
code of 3 used to give a pure-scalar quaternion); nothing is launched, the outputs keep their sentinels.
(The issue that asked for this file calls 27 "yxz"; in this packing 27 is the axis codes 3, 2, 1 and yxz is 33.  Both are refused.)

Found by this file: a joint that keeps its pose had lvrt = 8.8e-16 on the device (4.4e-16 at dt = 1/30, 1.8e-15 at 1/120, 1.3e-15 in
the xyz / yzx clips) where the reference has exactly 0.  The vector part of q q^-1 is w x - w x + (z y - y z); the compiler fused
the first product into the subtraction, fma(w, -x, round(w x)), which leaves the rounding residue of that product, and dq_to_helical
hands a vector below 1e-5 on unscaled.  rot_diff now multiplies through dq_mul_inv_unfused (every product rounded on its own, as NumPy
forms it): exactly 0 in all 29 clips.  No other kernel was wrong.

Measured on an MI355X (worst over the group; features: |got - ref| / (1 + |ref|)):
  features    float64 arrays   j1 3.2e-14   j3 7.2e-14 .. 5.5e-13   j24-root 2.6e-14 .. 2.1e-12   j64 / j65 7.0e-13 .. 1.2e-12
                               j130 2.2e-12 (N = 17), 9.5e-12 (N = 10)                                              bound 1e-9
              ltxy / ctxy      <= 8.4e-16: every float32 the oracle's                                               bound 1e-6
  channels    positions <= 1.4e-14, rotations <= 2.8e-15, angles <= 4.3e-13 degrees, all four branches              bounds 1e-9
  near poles  rotations 4.8e-14 (k = 1), 5.9e-13 (k = 2), 5.0e-12 (k = 3): about eps / cos(asin angle)              bound 1e-9
  at poles    asin angle 9.7e-4 (zyx), 9.3e-4 (xzy) degrees from +-90 -- the 1e-10 of the row normalisation, sin = 1 - 1e-10 -- and
              exactly 90 where |sin| > 1                                                                            bound 1e-3
  table       positions <= 1.6e-15, rotations <= 1.2e-15, angles <= 1.1e-13 degrees                                 bounds 1e-9
The 49 tests take 3.2 s in one process, the float64 oracle (its Python unroll loop included) and the clip builders in that time.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
from zeggs import anim, capi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
SENT = {torch.float64: -7.25e77, torch.float32: -3.5e33}
BVH_SHAPES = [(J, T) for J in (1, 3, 65) for T in (1, 2, 300)]
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _clip_and_oracle(case):
    def make():
        clip = H.anim_case_clip(case)
        return clip, H.anim_oracle(clip)
    return _cached(("features", H.anim_case_id(case)), make)


def _bvh(J, T):
    return _cached(("bvh", J, T), lambda: H.bvh_case(J, T, seed=100 * J + T))


def _guarded(n, dtype=torch.float64):
    buf = torch.full((n + 2 * PAD,), SENT[dtype], dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _guards_intact(buf):
    return bool((buf[:PAD] == SENT[buf.dtype]).all()) and bool((buf[-PAD:] == SENT[buf.dtype]).all())


def _untouched(buf):
    return bool((buf == SENT[buf.dtype]).all())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _last_error():
    return capi.raw().zeggs_last_error().decode()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ----------------------------------------------------------------------------- features
def _features_raw(clip, order=None):
    """zeggs_anim_features through the raw ABI into guarded views -> (rc, {name: (buffer, view)})"""
    names = clip["names"]
    N, J = clip["rotations"].shape[:2]
    d = capi.AnimDims(N, J, names.index("Hips"), names.index("Spine2"), names.index("Head"), float(clip["frametime"]),
                      anim.order_code(clip["order"]) if order is None else order)
    out, ptr = {}, capi.AnimOut()
    for n, w, dt in anim.ANIM_OUT:
        out[n] = _guarded(N * w if w > 0 else N * J * -w, dt)
        setattr(ptr, n, out[n][1].data_ptr())
    rot, pos, par = _dev(clip["rotations"], torch.float64), _dev(clip["positions"], torch.float64), _dev(clip["parents"], torch.int32)
    L = capi.raw()
    ws = torch.empty(int(L.zeggs_anim_features_workspace_bytes(C.byref(d))), dtype=torch.uint8, device=DEV)
    rc = L.zeggs_anim_features(C.byref(d), _p(par), _p(rot), _p(pos), C.byref(ptr), _p(ws), C.c_size_t(ws.numel()), ops._stream())
    torch.cuda.synchronize()
    return rc, out


def _check_features(case, got, ref, clip):
    errs = H.anim_errors(got, ref)
    print("ANIM features", H.anim_case_id(case), "f64 %.2e" % max(e for n, e in errs.items() if n not in ("ltxy", "ctxy")),
          "f32 %.2e" % max(errs["ltxy"], errs["ctxy"]))
    for n, e in errs.items():
        assert e <= H.anim_bound(n), (H.anim_case_id(case), n, e)
    s = H.anim_roles(case[0])["static"]
    if s is not None:
        lvrt = np.asarray(got[H.ANIM_FEATURES.index("lvrt")])
        print("ANIM static lvrt", H.anim_case_id(case), "%.2e" % np.abs(lvrt[:, s]).max())
        assert np.isfinite(lvrt).all() and (lvrt[:, s] == 0.0).all(), (H.anim_case_id(case), np.abs(lvrt[:, s]).max())
    if case[2].get("static_head"):
        gaze = np.asarray(got[H.ANIM_FEATURES.index("gaze_pos")])
        assert np.isfinite(gaze).all() and (gaze == gaze[0]).all()       # the median of N ties: that value (within the bound, above)


@pytest.mark.parametrize("case", [c for c in H.ANIM_CASES if c[0] != "j1"], ids=H.anim_case_id)
def test_features_equal_the_oracle(case):
    clip, ref = _clip_and_oracle(case)
    got = [t.cpu().numpy() for t in anim.preprocess_animation(clip, DEV)]
    _check_features(case, got, ref, clip)


@pytest.mark.parametrize("case", [("j1", 10, {}), ("j65", 17, {})], ids=H.anim_case_id)
def test_features_raw_abi_and_guards(case):
    """the one-joint rig (Hips = Spine2 = Head = 0), which only the raw ABI takes, and j65: the 16 arrays land in views of larger
    sentinel-filled buffers and the floats either side stay sentinels"""
    clip, ref = _clip_and_oracle(case)
    rc, out = _features_raw(clip)
    assert rc == 0, _last_error()
    shapes = [np.asarray(r).shape for r in ref]
    got = [out[n][1].cpu().numpy().reshape(s) for n, s in zip(H.ANIM_FEATURES, shapes)]
    _check_features(case, got, ref, clip)
    for n in H.ANIM_FEATURES:
        assert _guards_intact(out[n][0]), n


# axis codes: 3 | 1 << 2 | 2 << 4 (an axis 3), 27 (3, 2, 1), x x y, x y x, zyx with a bit above the three codes, negative
BAD_FROM_EULER = (39, 27, 16, 4, 6 | 64, -1)


def test_features_refuse_codes_that_are_no_channel_order():
    case = ("j3", 4, {})
    clip, ref = _clip_and_oracle(case)
    for code in BAD_FROM_EULER:
        rc, out = _features_raw(clip, order=code)
        msg = _last_error()
        assert rc == -1 and "anim_features" in msg and f"order code {code} " in msg and "permutation" in msg, (code, rc, msg)
        assert all(_untouched(out[n][0]) for n in H.ANIM_FEATURES), code
    with pytest.raises(ValueError, match="not a rotation channel order"):                # the wrapper raises what it raised
        anim.preprocess_animation(dict(clip, order="xxy"), DEV)
    shapes = [np.asarray(r).shape for r in ref]
    res = {}
    for code in (0, H.ANIM_ORDER_ZYX):                                                  # 0 remains zyx
        rc, out = _features_raw(clip, order=code)
        assert rc == 0, _last_error()
        res[code] = [out[n][1].cpu().numpy().reshape(s) for n, s in zip(H.ANIM_FEATURES, shapes)]
    _check_features(case, res[0], ref, clip)
    assert all((a == b).all() for a, b in zip(res[0], res[H.ANIM_ORDER_ZYX]))
    for name in ("yxz", "zxy"):                                                          # any permutation converts (from_euler takes any)
        c2 = H.anim_clip("j3", 4, seed=4, order=name)
        rc, out = _features_raw(c2)
        assert rc == 0, _last_error()
        got = [out[n][1].cpu().numpy().reshape(s) for n, s in zip(H.ANIM_FEATURES, shapes)]
        errs = H.anim_errors(got, H.anim_oracle(c2))
        assert all(e <= H.anim_bound(n) for n, e in errs.items()), (name, errs)


# ----------------------------------------------------------------------------- BVH conversion
def _check_channels(tag, pos, eul, opos, oeul, order, branch=None, need_all=False):
    assert np.isfinite(pos).all() and np.isfinite(eul).all(), tag
    pe = float(np.max(np.abs(pos - opos) / (1.0 + np.abs(opos))))
    qe, ae = H.euler_quat_error(eul, oeul, order), H.euler_angle_error(eul, oeul, order)
    print("ANIM bvh", tag, "pos %.2e quat %.2e angle %.2e" % (pe, qe.max(), ae.max()))
    assert pe <= H.BVH_POS_BOUND, (tag, pe)
    if branch is None:
        assert qe.max() <= H.BVH_QUAT_BOUND and ae.max() <= H.BVH_ANGLE_BOUND, (tag, qe.max(), ae.max())
        return
    for b in range(4):
        items = branch == b
        assert items.sum() >= (8 if need_all else 0), (tag, b, int(items.sum()))
        if items.any():
            assert qe[items].max() <= H.BVH_QUAT_BOUND and ae[items].max() <= H.BVH_ANGLE_BOUND, (tag, b, qe[items].max(), ae[items].max())


def _channels(x, order, start):
    kw = {} if start is None else dict(start_position=start[0], start_rotation=start[1])
    pos, eul = anim.bvh_channels(_dev(x["root_pos"]), _dev(x["root_rot"]), _dev(x["lpos"]), _dev(x["ltxy"]), order=order, **kw)
    return pos.cpu().numpy(), eul.cpu().numpy()


@pytest.mark.parametrize("J,T", BVH_SHAPES)
def test_bvh_channels_equal_the_oracle(J, T):
    x = _bvh(J, T)
    for order in ("zyx", "xzy"):
        for sname, start in H.BVH_STARTS.items():
            pos, eul = _channels(x, order, start)
            opos, oeul = H.bvh_oracle(x, order, start)
            _check_channels(f"J{J}-T{T}-{order}-{sname}", pos, eul, opos, oeul, order, x["branch"], need_all=T * J >= 32)
    with pytest.raises(NotImplementedError, match="Cannot convert to ordering"):          # the wrapper raises what it raised
        _channels(x, "yxz", None)


@pytest.mark.parametrize("order", ["zyx", "xzy"])
def test_bvh_channels_near_the_poles(order):
    mid = H.BVH_ASIN_OUTPUT[order]
    for k in (1, 2, 3):
        x = H.bvh_pole_case(order, k)
        pos, eul = _channels(x, order, None)
        opos, oeul = H.bvh_oracle(x, order)
        assert np.abs(np.abs(eul[..., mid]) - (90.0 - 10.0 ** -k)).max() < 5e-4
        _check_channels(f"pole-k{k}-{order}", pos, eul, opos, oeul, order)


@pytest.mark.parametrize("order", ["zyx", "xzy"])
def test_bvh_channels_at_the_poles(order):
    """asin angle +-90 degrees exactly: the other two angles are undetermined (the oracle's own round trip is off by 0.7 in a
    quaternion component there), so only: finite, the asin angle within 1e-3 degrees of +-90, and no NaN where |sin| rounds above 1
    (joint 0: 90 exactly)"""
    mid = H.BVH_ASIN_OUTPUT[order]
    x = H.bvh_pole_case(order, None)
    assert (np.abs(H.bvh_raw_sin(x, order)[:, 0]) > 1.0).all()
    pos, eul = _channels(x, order, None)
    assert np.isfinite(eul).all() and np.isfinite(pos).all()
    off = np.abs(np.abs(eul[..., mid]) - 90.0)
    print("ANIM bvh exact pole", order, "%.2e" % off.max())
    assert off.max() < 1e-3 and (off[:, 0] == 0.0).all()
    assert (np.sign(eul[..., mid]) == np.sign(x["middle"])).all()


def _bvh_dims(T, J, order, start):
    d = capi.BvhDims(T, J, int(start is not None))
    d.order = order
    if start is not None:
        d.start_pos[:], d.start_rot[:] = [float(v) for v in start[0]], [float(v) for v in start[1]]
    return d


def _pose_to_bvh_raw(x, order, start):
    T, J = x["lpos"].shape[:2]
    d = _bvh_dims(T, J, order, start)
    (pb, pv), (eb, ev) = _guarded(T * J * 3), _guarded(T * J * 3)
    ins = [_dev(x[k]) for k in ("root_pos", "root_rot", "lpos", "ltxy")]
    rc = capi.raw().zeggs_pose_to_bvh(C.byref(d), *[_p(t) for t in ins], _p(pv), _p(ev), ops._stream())
    torch.cuda.synchronize()
    return rc, pb, eb, pv.cpu().numpy().reshape(T, J, 3), ev.cpu().numpy().reshape(T, J, 3)


def _table_raw(x, seq, order, start, t0, t1, ref):
    """rows [t0, t1) of the clip through zeggs_pose_to_bvh_table into a guarded view; ref: pass the clip's frame 0 / NULL"""
    J = x["lpos"].shape[1]
    d = _bvh_dims(t1 - t0, J, order, start)
    buf, view = _guarded((t1 - t0) * (3 + 3 * J))
    ins = [_dev(x[k][t0:t1]) for k in ("root_pos", "root_rot", "lpos", "ltxy")]
    refs = [_dev(x["root_pos"][:1]), _dev(x["root_rot"][:1])] if ref else [None, None]
    sq = _dev(np.asarray(seq, np.int32))
    rc = capi.raw().zeggs_pose_to_bvh_table(C.byref(d), *[_p(t) for t in ins], _p(refs[0]), _p(refs[1]), _p(sq), _p(view), ops._stream())
    torch.cuda.synchronize()
    return rc, buf, view.cpu().numpy().reshape(t1 - t0, 3 + 3 * J)


@pytest.mark.parametrize("J,T", [(3, 2), (65, 300)])
def test_pose_to_bvh_raw_abi_and_guards(J, T):
    x = _bvh(J, T)
    for order, code in (("zyx", 0), ("zyx", H.ANIM_ORDER_ZYX), ("xzy", H.ANIM_ORDER_XZY)):
        rc, pb, eb, pos, eul = _pose_to_bvh_raw(x, code, H.BVH_START)
        assert rc == 0, _last_error()
        opos, oeul = H.bvh_oracle(x, order, H.BVH_START)
        _check_channels(f"raw-J{J}-T{T}-code{code}", pos, eul, opos, oeul, order, x["branch"])
        assert _guards_intact(pb) and _guards_intact(eb)


@pytest.mark.parametrize("J", [3, 65])
def test_table_equals_the_oracle(J):
    T = 20
    x, seq = _bvh(J, T), H.bvh_table_seq(J)
    assert seq[0] != 0 and sum(s != i for i, s in enumerate(seq)) * 2 >= J
    for order, code in (("zyx", H.ANIM_ORDER_ZYX), ("xzy", H.ANIM_ORDER_XZY)):
        for start in (None, H.BVH_START):
            # the whole clip without a reference, then the three chunks with the clip's frame 0 as reference
            for t0, t1, ref in ((0, T, False), (0, 7, True), (7, 8, True), (8, T, True)):
                rc, buf, table = _table_raw(x, seq, code, start, t0, t1, ref)
                assert rc == 0, _last_error()
                want = H.bvh_table_expected(x, seq, order, start, t0, t1)
                pe, qe, ae = H.bvh_table_errors(table, want, order)
                print("ANIM table", f"J{J}-{order}-{'start' if start else 'nostart'}-[{t0},{t1})", "pos %.2e quat %.2e angle %.2e" % (pe, qe, ae))
                assert pe <= H.BVH_POS_BOUND and qe <= H.BVH_QUAT_BOUND and ae <= H.BVH_ANGLE_BOUND, (J, order, t0, t1, pe, qe, ae)
                assert _guards_intact(buf)


BAD_TO_EULER = (27, 33, 1, 9, 6 | 64, -1)        # 33 = yxz, 9 = yzx: channel orders, but not ones quat.to_euler has


def test_bvh_entry_points_refuse_orders_they_cannot_convert():
    x, seq = _bvh(3, 2), H.bvh_table_seq(3)
    for code in BAD_TO_EULER:
        rc, pb, eb, _, _ = _pose_to_bvh_raw(x, code, None)
        msg = _last_error()
        assert rc == -1 and msg.startswith("pose_to_bvh:") and f"order code {code}:" in msg and "only zyx" in msg and "xzy" in msg, (code, rc, msg)
        assert _untouched(pb) and _untouched(eb), code
        rc, buf, _ = _table_raw(x, seq, code, None, 0, 2, False)
        msg = _last_error()
        assert rc == -1 and msg.startswith("pose_to_bvh_table:") and f"order code {code}:" in msg and "only zyx" in msg and "xzy" in msg, (code, rc, msg)
        assert _untouched(buf), code
    with pytest.raises(RuntimeError, match="pose_to_bvh.*order code 27"):                  # the typed handle raises the message
        d = _bvh_dims(2, 3, 27, None)
        t = torch.zeros(2 * 3 * 3, dtype=torch.float64, device=DEV)
        capi.api().zeggs_pose_to_bvh(d, *[_dev(x[k]) for k in ("root_pos", "root_rot", "lpos", "ltxy")], t, t.clone(), ops._stream())
