"""Left/right mirroring on the device: the signed column gather (csrc/mirror.hip, include/zeggs_hip_mirror.h) against NumPy, bit for
bit; the dataset builder with `mirror` against the same corpus with the mirrored files written out; the device features of a
mirrored take against the mirrored features; mirror_processed; generation from a mirrored exemplar.

Kernel: cols 1, 63, 64, 65, 225, 1137 (and 3072, the widest a plan takes: tiles of four float32 / two float64 rows) x rows 1, 2, 257
(and 9001 at 225 columns: more tiles than one workgroup's first pass, a last tile that is not full), float32 and float64, 16-byte
aligned tables (the vector path) and tables one element off (the element path); identity, all-negated, column reversal and a seeded
random signed involution; inputs with -0.0, +-inf and NaNs with payloads.  The expected table is the exclusive-or on the integer
view (anim.mirror_rows_host), so every comparison is of bytes.  Destinations are views into sentinel buffers that must be intact
either side.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import helpers as H
from zeggs import anim, capi, data_pipeline, generate, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
COLS = (1, 63, 64, 65, 225, 1137)
ROWS = (1, 2, 257)


def _tables(cols, seed):
    rng = np.random.default_rng(seed)
    u = lambda src, neg: (np.asarray(src, np.uint32) | (np.asarray(neg, np.uint32) << 31)).view(np.int32)  # noqa: E731
    ident = u(np.arange(cols), np.zeros(cols))
    negated = u(np.arange(cols), np.ones(cols))
    reverse = u(np.arange(cols)[::-1], np.zeros(cols))
    order = rng.permutation(cols)
    src, neg = np.arange(cols), np.zeros(cols, np.uint32)
    i = 0
    while i < cols:                                  # pairs (three in four) and fixed points, a pair shares its sign
        s = rng.integers(2)
        if i + 1 < cols and rng.integers(4):
            a, b = order[i], order[i + 1]
            src[a], src[b], neg[a], neg[b] = b, a, s, s
            i += 2
        else:
            neg[order[i]] = s
            i += 1
    return dict(identity=ident, negated=negated, reversal=reverse, involution=u(src, neg))


def _input(rows, cols, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, cols)).astype(dtype)
    bits = x.view({4: np.uint32, 8: np.uint64}[x.itemsize]).reshape(-1)
    special = {4: [0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0],
               8: [1 << 63, 0x7FF << 52, 0xFFF << 52, (0x7FF8 << 48) | 1, (0xFFF8 << 48) | 0x123456789ABC, (0x7FF << 52) | 1, 1, 0]}[x.itemsize]
    where = rng.permutation(bits.size)[:max(1, min(bits.size // 5, 4096))]
    bits[where] = np.asarray(special, bits.dtype)[np.arange(where.size) % 8]
    return x


def _guarded(x, offset):
    """x on the device inside a buffer of sentinels, `offset` elements past a 16-byte boundary -> (buffer, view)"""
    n = x.size
    buf = torch.full((n + 2 * PAD + 4,), -7.25e33, dtype=torch.from_numpy(x).dtype, device=DEV)
    view = buf[PAD + offset:PAD + offset + n].view(x.shape)
    view.copy_(torch.from_numpy(x))
    return buf, view


def _edges_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == -7.25e33).all()) and bool((buf[lo + view.numel():] == -7.25e33).all())


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _rows_raw(plan, src, dst, rows, eb):
    return capi.raw().zeggs_mirror_rows(plan, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_long(rows), eb, ops._stream())


# ----------------------------------------------------------------------------- 1. the kernel against NumPy
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cols", COLS + (3072,))
def test_kernel_equals_numpy_bit_for_bit(cols, dtype):
    shapes = [(r, 0) for r in ROWS] + [(2, 1), (257, 1)] + ([(9001, 0), (9001, 1)] if cols == 225 else [])
    for kind, table in _tables(cols, cols).items():
        plan = anim._MirrorPlan(table)
        assert capi.api().zeggs_mirror_plan_cols(plan.handle) == cols
        for rows, offset in shapes if kind == "involution" else shapes[:3]:
            x = _input(rows, cols, dtype, seed=rows + cols)
            want = anim.mirror_rows_host(x, table)
            in_buf, xin = _guarded(x, offset)
            out_buf, out = _guarded(np.zeros_like(x), offset)
            out.fill_(-7.25e33)
            assert (xin.data_ptr() % 16 == 0) == (offset == 0)
            assert _rows_raw(plan.handle, xin, out, rows, x.itemsize) == 0, capi.raw().zeggs_last_error()
            torch.cuda.synchronize()
            assert _bytes(out) == want.tobytes(), (kind, rows, offset)
            assert _bytes(xin) == x.tobytes() and _edges_intact(out_buf, out) and _edges_intact(in_buf, xin)
            if kind == "involution":                 # twice is the identity, on the device too
                back = anim.mirror_rows(out.clone(), table)
                assert _bytes(back) == x.tobytes()


def test_rows_zero_overlap_and_bad_tables_launch_nothing():
    table = _tables(65, 1)["involution"]
    plan = anim._MirrorPlan(table)
    x = _input(8, 65, np.float32, 3)
    buf, view = _guarded(np.concatenate([x, x]), 0)
    before = _bytes(buf)
    L = capi.raw()
    assert _rows_raw(plan.handle, view[:8], view[8:], 0, 4) == 0                       # rows = 0: a no-op
    flat = view.reshape(-1)
    for src, dst, rows, eb, msg in ((view[:8], view[:8], 8, 4, "overlap"), (view[:8], flat[65:], 8, 4, "overlap"), (flat[65:], view[:8], 8, 4, "overlap"),
                                    (view[:8], flat[8 * 65 - 1:], 8, 4, "overlap"), (view[:8], view[8:], 8, 2, "elements of 2 bytes"),
                                    (view[:8], view[8:], -1, 4, "-1 rows"), (flat[1:], view[8:], 4, 8, "not aligned")):
        assert _rows_raw(plan.handle, src, dst, rows, eb) == -1
        assert msg in L.zeggs_last_error().decode()
    no_plan = np.zeros(8, np.int64)                                                    # (host memory that is no plan)
    assert L.zeggs_mirror_rows(C.c_void_p(no_plan.ctypes.data), C.c_void_p(view.data_ptr()), C.c_void_p(view[8:].data_ptr()), C.c_long(1), 4, None) == -1
    assert "not a plan" in L.zeggs_last_error().decode()
    handle = C.c_void_p(77)
    for bad, msg in ((np.array([0, 0, 1], np.int32), "not a bijection"), (np.array([0, 3, 1], np.int32), "source 3 of 3 columns")):
        assert L.zeggs_mirror_plan_create(C.c_void_p(bad.ctypes.data), 3, C.byref(handle)) == -1 and handle.value is None
        assert msg in L.zeggs_last_error().decode()
        with pytest.raises(RuntimeError, match=msg):
            anim.mirror_rows(view[:8, :3].contiguous(), bad)
    torch.cuda.synchronize()
    assert _bytes(buf) == before                                                       # nothing was written anywhere
    with pytest.raises(ValueError, match="does not hold rows of 65 columns"):
        anim.mirror_rows(view[:8, :64].contiguous(), table)
    with pytest.raises(RuntimeError, match="on the GPU"):
        anim.mirror_rows(torch.zeros(2, 65), table)
    assert anim.mirror_rows(torch.zeros(0, 65, device=DEV), table).shape == (0, 65)


def test_mirror_take_on_the_device_equals_the_host():
    clip = synth.make_bvh_clip(33, seed=4)
    host = anim.mirror_take(clip)
    for dt in (torch.float32, torch.float64):
        dev = anim.mirror_take(dict(clip, rotations=torch.as_tensor(clip["rotations"]).to(DEV, dt), positions=torch.as_tensor(clip["positions"]).to(DEV, dt)))
        for k in ("rotations", "positions"):
            assert dev[k].is_cuda and _bytes(dev[k]) == host[k].astype(dev[k].cpu().numpy().dtype).tobytes()
        assert dev["offsets"].tobytes() == host["offsets"].tobytes() and dev["asymmetry"] == host["asymmetry"]


# ----------------------------------------------------------------------------- 2. the dataset builder
def _corpus():
    return [synth.make_raw_take("a_Happy", 70, seed=1, style="Happy"), synth.make_raw_take("b_Sad", 64, seed=2, style="Sad", validation=True),
            synth.make_raw_take("c_Happy", 58, seed=3, style="Happy")]


def _run_a_and_b(tmp_path_factory):
    """A: the corpus with mirror: true.  B: the same corpus with the mirrored BVH files written by mirror_take + bvh_save and listed
    in the info CSV directly after their originals, no `mirror` key.  -> (A's results, B's results, A's folder, B's folder)"""
    def make():
        a_dir, b_dir = tmp_path_factory.mktemp("mirror_a"), tmp_path_factory.mktemp("mirror_b")
        takes = _corpus()
        synth.write_raw_corpus(a_dir, takes)
        synth.write_raw_corpus(b_dir, takes)
        doubled = []
        for t in takes:
            loaded = anim.bvh_load(str(b_dir / "original" / (t["name"] + ".bvh")))
            anim.bvh_save(b_dir / "original" / (t["name"] + "_mirror.bvh"), anim.mirror_take(loaded))
            doubled += [t["info"], dict(t["info"], anim_bvh=t["name"] + "_mirror.bvh")]
        import csv
        with open(b_dir / "info.csv", "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=synth.INFO_COLUMNS)
            w.writeheader()
            w.writerows(doubled)
        ratios = [0.9, 1.0, 1.1]
        a = data_pipeline.data_pipeline(synth.pipeline_conf(a_dir, len_ratios=ratios, mirror=True))
        b = data_pipeline.data_pipeline(synth.pipeline_conf(b_dir, len_ratios=ratios))
        return a, b, a_dir, b_dir
    return H._live_cached("mirror_pipeline_runs", make)


def test_pipeline_with_mirror_equals_the_pipeline_over_mirrored_files(tmp_path_factory):
    (pa, da), (pb, db), a_dir, b_dir = _run_a_and_b(tmp_path_factory)
    assert len(pa["ranges_train"]) == 2 * 2 * 3 and len(pa["ranges_valid"]) == 2 * 1 * 3              # takes x (capture, reflection) x ratios
    assert set(pa) == set(pb) and da == db
    for k in pa:
        assert np.asarray(pa[k]).dtype == np.asarray(pb[k]).dtype and np.array_equal(pa[k], pb[k]), k
    for name in ("processed_data.npz", "stats.npz"):
        za, zb = np.load(a_dir / "processed" / name), np.load(b_dir / "processed" / name)
        assert set(za.files) == set(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files), name
    assert (a_dir / "processed" / "data_definition.json").read_bytes() == (b_dir / "processed" / "data_definition.json").read_bytes()
    fa = sorted(p.relative_to(a_dir) for p in (a_dir / "processed" / "trimmed").rglob("*") if p.is_file())
    fb = sorted(p.relative_to(b_dir) for p in (b_dir / "processed" / "trimmed").rglob("*") if p.is_file())
    assert fa == fb and len(fa) == 3 * 2 * 3 * 2                                                          # takes x sides x ratios x (bvh, wav)
    for rel in fa:
        assert (a_dir / rel).read_bytes() == (b_dir / rel).read_bytes(), rel
    conf = json.loads((a_dir / "processed" / "data_pipeline_conf.json").read_text())
    assert conf["mirror"] is True and "mirror" not in json.loads((b_dir / "processed" / "data_pipeline_conf.json").read_text())
    # the reflection is a reflection: its rows are the table applied to the capture's, to the bounds of the feature kernels (below)
    s, e = pa["ranges_train"][0]
    ms, me = pa["ranges_train"][3]
    assert e - s == me - ms and np.array_equal(pa["X_audio_features"][s:e], pa["X_audio_features"][ms:me])
    assert not np.array_equal(pa["Y_lpos"][s:e], pa["Y_lpos"][ms:me])


def test_rows_already_mirrored_are_not_mirrored_again(tmp_path_factory):
    """B's corpus with mirror: true lists every reflection already: the same dataset again"""
    (pa, _), _, _, b_dir = _run_a_and_b(tmp_path_factory)
    conf = synth.pipeline_conf(b_dir, len_ratios=[0.9, 1.0, 1.1], mirror={"suffix": "_mirror"}, processed_data_path="again", save_final_data=False)
    again, _ = data_pipeline.data_pipeline(conf)
    assert set(again) == set(pa) and all(np.array_equal(again[k], pa[k]) for k in pa)
    assert not (b_dir / "again" / "processed_data.npz").exists()


def test_mirror_processed_equals_the_pipeline(tmp_path_factory):
    """run A's un-mirrored half -> mirror_processed -> run A's dataset.  Ranges, labels and the audio rows are equal; every Y_* array
    and every statistic is within the bounds tests/test_gpu_anim_dims.py applies to the feature arrays (helpers.ANIM_F64_BOUND, for
    ltxy helpers.ANIM_F32_BOUND, as |a - b| / (1 + |b|)), unchanged -- but for the three gaze-direction columns at the end of
    anim_input_mean / anim_input_std.  The dataset does not store the gaze direction; mirror_processed restates it from the stored
    FLOAT32 root and gaze rows where the pipeline has them in float64, so those six numbers get a float32-rounding bound of their
    own, absolute: with R = max |gaze_pos| + max |root_pos|, the difference vector is off by 2^-24 R (its two rounded operands), the
    rotation by the rounded quaternion by at most 4 x 2^-24 R (four components, each entering twice), the float32 store of the
    direction and the float32 store of the statistic by 2^-24 R each -- 7 x 2^-24 R, taken as 8 x 2^-24 R; a mean moves by no more
    than its elements do, and neither does the pooled deviation."""
    (pa, da), _, _, _ = _run_a_and_b(tmp_path_factory)
    keep = lambda r: [tuple(x) for i, x in enumerate(r.tolist()) if (i // 3) % 2 == 0]  # noqa: E731   (three ratios a take, captures first)
    spans = sorted(keep(pa["ranges_train"]) + keep(pa["ranges_valid"]))
    half, row = {k: np.concatenate([pa[k][s:e] for s, e in spans]) for k in data_pipeline._PROCESSED_KEYS}, 0
    new_of = {}
    for s, e in spans:
        new_of[(s, e)] = [row, row + e - s]
        row += e - s
    pick = lambda r, lab: (np.asarray([new_of[x] for x in keep(r)], np.int32).reshape(-1, 2), lab[[i for i in range(len(lab)) if (i // 3) % 2 == 0]])  # noqa: E731
    half["ranges_train"], half["ranges_train_labels"] = pick(pa["ranges_train"], pa["ranges_train_labels"])
    half["ranges_valid"], half["ranges_valid_labels"] = pick(pa["ranges_valid"], pa["ranges_valid_labels"])
    got, definition = data_pipeline.mirror_processed(half, da, ranges_per_take=3)
    assert definition == da and set(got) == set(pa)
    assert data_pipeline._IN_STATS[-1] == "Y_gaze_dir"
    reach = float(np.abs(pa["Y_gaze_pos"]).max() + np.abs(pa["Y_root_pos"]).max())
    gaze_bound, worst = 8 * 2.0 ** -24 * reach, {}
    for k in pa:
        a, b = np.asarray(got[k]), np.asarray(pa[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.startswith("ranges") or k == "X_audio_features":
            assert np.array_equal(a, b), k
            continue
        a, b = a.astype(np.float64), b.astype(np.float64)
        if k in ("anim_input_mean", "anim_input_std"):            # (..., Y_gaze_dir: the last three columns)
            worst[k + "[gaze_dir]"] = float(np.abs(a[-3:] - b[-3:]).max())
            a, b = a[:-3], b[:-3]
        worst[k] = float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))
    print("mirror_processed against the pipeline, worst |a - b| / (1 + |b|) (gaze_dir: |a - b|, bound %.2e):" % gaze_bound,
          {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= (gaze_bound if k.endswith("[gaze_dir]") else H.ANIM_F32_BOUND if "ltxy" in k else H.ANIM_F64_BOUND), (k, v)
    with pytest.raises(ValueError, match="not whole takes"):
        data_pipeline.mirror_processed(half, da, ranges_per_take=2)


# ----------------------------------------------------------------------------- 3. the device features commute with the mirror
@pytest.mark.parametrize("order", ["zyx", "xzy", "yzx"])
def test_device_features_of_a_mirrored_take_are_the_mirrored_features(order):
    """preprocess_animation_device of the mirrored take against mirror_rows of the features of the original, per array within the
    bounds tests/test_gpu_anim_dims.py applies to these arrays against the oracle (helpers.anim_errors / anim_bound)"""
    clip = synth.make_bvh_clip(97, seed=11)
    clip["order"] = order
    pairs = anim.mirror_pairs(clip["names"], clip["parents"])
    plain = anim.preprocess_animation(clip, DEV)
    mirrored = anim.preprocess_animation(anim.mirror_take(clip), DEV)
    via = [anim.mirror_rows(a, n, pairs) for n, a in zip(H.ANIM_FEATURES, plain)]
    errs = H.anim_errors([t.cpu().numpy() for t in mirrored], [t.cpu().numpy() for t in via])
    diff = {n: float((a.double() - b.double()).abs().max()) for n, a, b in zip(H.ANIM_FEATURES, mirrored, via)}
    print("MIRROR commute", order, json.dumps({n: diff[n] for n in H.ANIM_FEATURES}))
    for n, e in errs.items():
        assert e <= H.anim_bound(n), (order, n, e)
    assert all(not torch.equal(a, b) for a, b in zip(plain, mirrored))


# ----------------------------------------------------------------------------- 4. generation
def test_generation_from_a_mirror_entry_equals_generation_from_the_mirrored_file(golden_dir, tmp_path):
    """generate_gesture with (bvh, frames, "mirror") and with mirror_style=True against generate_gesture given the mirrored exemplar
    file: the same encoding and the same BVH, bit for bit (same seed and temperature; the encoder's products in a fixed summation
    order, without which two runs of ONE call differ in the last place).  generate_gestures: the job with Job(mirror_style=True)
    against the job given the mirrored file in the same call, the same bytes, and not those of the job without the switch.  A
    mirror request on an embedding entry is refused."""
    import test_gpu_text as gt
    net, data, ex, wavfile = gt._generate_fixture(golden_dir, tmp_path)
    wavfile.write(tmp_path / "a.wav", 16000, synth.synth_wav(17067, seed=31))          # 64 frames
    mex = tmp_path / "ex_mirror.bvh"
    anim.bvh_save(mex, anim.mirror_take(anim.bvh_load(str(ex))))
    kw = dict(style_encoding_type="example", blend_type="add", blend_ratio=[1.0], first_pose=ex, temperature=0.7, seed=77)
    res = tmp_path / "res"
    with ops.fixed_order_gemms():
        want = generate.generate_gesture(tmp_path / "a.wav", [(mex, (5, 60))], net, data, res, file_name="file", **kw)
        plain = generate.generate_gesture(tmp_path / "a.wav", [(ex, (5, 60))], net, data, res, file_name="plain", **kw)
        entry = generate.generate_gesture(tmp_path / "a.wav", [(ex, (5, 60), "mirror")], net, data, res, file_name="entry", **kw)
        switch = generate.generate_gesture(tmp_path / "a.wav", [(ex, (5, 60))], net, data, res, file_name="switch", mirror_style=True, **kw)
        job = generate.Job(tmp_path / "a.wav", [(ex, (5, 60))], file_name="job", first_pose=ex, temperature=0.7, seed=77, blend_ratio=[1.0], mirror_style=True)
        mk = lambda style, name, **k: generate.Job(tmp_path / "a.wav", [style], file_name=name, first_pose=ex, temperature=0.7, seed=77,  # noqa: E731
                                                   blend_ratio=[1.0], **k)
        generate.generate_gestures([job, mk((mex, (5, 60)), "job_file"), mk((ex, (5, 60)), "job_plain"), mk((ex, (5, 60), "mirror"), "job_entry")],
                                   net, data, res, batch=1)
        single = generate.generate_gesture(tmp_path / "a.wav", [(mex, (5, 60))], net, data, res, file_name="file1", **kw)
    assert _bytes(entry) == _bytes(want) and _bytes(switch) == _bytes(want) and _bytes(plain) != _bytes(want) and _bytes(single) == _bytes(want)
    file = (res / "file.bvh").read_bytes()
    assert (res / "entry.bvh").read_bytes() == file and (res / "switch.bvh").read_bytes() == file and (res / "plain.bvh").read_bytes() != file
    job_file = (res / "job_file.bvh").read_bytes()
    assert (res / "job.bvh").read_bytes() == job_file and (res / "job_entry.bvh").read_bytes() == job_file
    assert (res / "job_plain.bvh").read_bytes() != job_file
    with pytest.raises(ValueError, match="mirror.*embedding"):
        generate.generate_gesture(None, [(np.zeros(64, np.float32), "vec")], net, data, None, mirror_style=True, **kw)
    with pytest.raises(ValueError, match="third field"):
        generate.generate_gesture(None, [(ex, None, "flip")], net, data, None, **kw)


def test_add_style_mirror_equals_the_mirrored_file(tmp_path):
    import test_gpu_live_styles as ls
    srv = ls._server(1, 4, styles=dict(net=ls._style_net(), capacity=4))
    clip = synth.make_bvh_clip(90, seed=9)
    anim.bvh_save(tmp_path / "c.bvh", clip)
    anim.bvh_save(tmp_path / "m.bvh", anim.mirror_take(anim.bvh_load(str(tmp_path / "c.bvh"))))
    a = srv.add_style("switch", str(tmp_path / "c.bvh"), trim=(3, 80), mirror=True)
    b = srv.add_style("file", str(tmp_path / "m.bvh"), trim=(3, 80))
    c = srv.add_style("plain", str(tmp_path / "c.bvh"), trim=(3, 80))
    d = srv.add_style("clip", anim.bvh_load(str(tmp_path / "c.bvh")), trim=(3, 80), mirror=True)
    rows = [np.concatenate(ops.live_style_read(srv._sb, slot=s)) for s in (a, b, c, d)]
    assert rows[0].tobytes() == rows[1].tobytes() == rows[3].tobytes() and rows[0].tobytes() != rows[2].tobytes()
    with pytest.raises(ValueError, match="mirror reflects an example's BVH channels"):
        srv.add_style("v", np.zeros(64, np.float32), mirror=True)
