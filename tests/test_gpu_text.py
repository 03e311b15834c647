"""The BVH motion text formatted on the device (csrc/text.hip: zeggs_table_text_device; anim.format_rows_device and the writers on
top of it).  The oracle is the host's snprintf("%f") on the same table (anim.format_rows): the comparison is == on bytes, and the
row ends are checked against the host's line ends."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import helpers
from zeggs import anim, generate, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# The library scans row lengths in blocks of 256 rows (one row per thread), measures a row per 64-lane wave and emits a row per
# 256-lane workgroup, 256 columns at a time.  (1, 1): one lane; (1, 228): one real row; (3, 3): a row that ends inside a wave;
# (7, 65): a row that crosses a wave; (257, 228): rows across a scan block; (5, 1027): more columns than a workgroup has lanes
# (four full emit steps and a short one); (4099, 7): many scan blocks; (65793, 1): more scan blocks than ONE step of the scan over
# the block totals holds (256 * 256 rows -- added to the issue's list because the totals are scanned 256 at a time); (0, 228): empty.
SHAPES = [(1, 1), (1, 228), (3, 3), (7, 65), (257, 228), (5, 1027), (4099, 7), (65793, 1), (0, 228)]
SPECIALS = [-0.0, 0.9999995, 9.9999995, -99.9999995, 0.0078125, 5e-324, 999999999999999.9]


def mixed_table(rows, cols, seed):
    """a seeded mix of every value class of tests/host/text_format_check.cpp, interleaved so that the widths within a row differ,
    with the issue's special values placed over it"""
    rng = np.random.default_rng(seed)
    n = rows * cols
    k = rng.integers(-2000000, 2000001, n).astype(np.float64)
    bits = (rng.integers(0, 1 << 52, n, dtype=np.uint64) | (rng.integers(900, 1072, n, dtype=np.uint64) << np.uint64(52)) |
            (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)))
    classes = [
        bits.view(np.float64),                                                       # random bit patterns inside the domain
        (rng.random(n) - 0.5) * 720.0,                                               # degrees
        ((rng.random(n) - 0.5) * 400.0).astype(np.float32).astype(np.float64),       # float32 origin
        k / 128.0,                                                                   # exact ties
        np.ldexp(k, -7 - rng.integers(0, 20, n)),                                    # ties k * 2^-7..-26
        (k + 0.5) * 1e-6,
        np.trunc(k / 1000.0) + np.where(k < 0, -0.9999995, 0.9999995),               # carries
        (rng.integers(0, 1 << 52, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))).view(np.float64),   # subnormals, +-0
        np.ldexp(rng.random(n), rng.integers(0, 50, n)) * rng.choice([-1.0, 1.0], n),                  # up to 2^50
    ]
    pick = (np.arange(n) + rng.integers(0, 3, n)) % len(classes)
    t = np.choose(pick, classes)
    if n:
        at = rng.permutation(n)[:min(n, 3 * len(SPECIALS))]
        t[at] = np.resize(np.asarray(SPECIALS), len(at))
    t = t.reshape(rows, cols)
    assert not n or (np.isfinite(t).all() and np.abs(t).max() < 1e15)
    return np.ascontiguousarray(t)


def host_text(table):
    """-> (bytes, line ends) from the host formatter"""
    txt = anim.format_rows(table) if table.shape[0] else b""
    ends = np.flatnonzero(np.frombuffer(txt, np.uint8) == 10) + 1
    assert len(ends) == table.shape[0]
    return txt, ends


def raw_call(table_dev, cap, guard=0):
    """zeggs_table_text_device on a text buffer with `guard` bytes of 0xA5 on either side -> (buffer, row_end, status, rc)"""
    rows, cols = table_dev.shape
    L = ops.lib()
    L.zeggs_table_text_workspace_bytes.restype = C.c_size_t
    buf = torch.full((cap + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    row_end = torch.full((max(rows, 1),), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nws = int(L.zeggs_table_text_workspace_bytes(C.c_long(rows), int(cols)))
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
    rc = L.zeggs_table_text_device(C.c_void_p(table_dev.data_ptr()), C.c_long(rows), int(cols), C.c_void_p(buf.data_ptr() + guard),
                                   C.c_size_t(cap), C.c_void_p(row_end.data_ptr()), C.c_void_p(status.data_ptr()),
                                   C.c_void_p(ws.data_ptr()), C.c_size_t(nws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), row_end.cpu().numpy(), int(status.item()), rc


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_device_text_equals_snprintf(rows, cols):
    """every shape, both emit variants: the bytes and the row ends of the host formatter"""
    table = mixed_table(rows, cols, seed=1000 * rows + cols)
    want, ends = host_text(table)
    dev = torch.as_tensor(table, device=DEV).reshape(rows, cols)
    try:
        for emit in (0, 1):
            ops.set_option("text_emit", emit)
            cap = rows * (cols * 24 + 1)
            buf, row_end, status, rc = raw_call(dev, cap)
            assert rc == 0 and status == 0, (emit, rc, status)
            if rows == 0:
                assert (buf == 0xA5).all() and (row_end == -7).all()          # touches nothing
                continue
            assert np.array_equal(row_end, ends), emit
            assert buf[:len(want)].tobytes() == want, emit
            assert (buf[len(want):] == 0xA5).all(), emit
    finally:
        ops.set_option("text_emit", 0)
    pieces = anim.format_rows_device(dev)
    assert len(pieces) == 1 and bytes(pieces[0]) == want


def _rollout_table(T=40):
    """the rows zeggs_pose_to_bvh_table makes from a short synthetic rollout (inputs as tests/test_gpu_batch_decode.py builds them)"""
    stats = synth.make_stats()
    c = synth.make_clip(T, seed=4, stats=stats)
    J = c["Y_lpos"].shape[1]
    g = lambda k: torch.as_tensor(np.ascontiguousarray(c[k][:T]), dtype=torch.float32, device=DEV).contiguous()  # noqa: E731
    rpos, rrot, lpos, ltxy = g("Y_root_pos"), g("Y_root_rot"), g("Y_lpos"), g("Y_ltxy")
    _, seq = anim.bvh_header(np.zeros((J, 3)), synth.PARENTS, synth.BONE_NAMES, "zyx", T, synth.DT)
    seq_dev = torch.as_tensor(np.asarray(seq, np.int32), device=DEV)
    d = anim.BvhDims(T, J, 1)
    d.start_pos[:] = [0.0, 0.0, 0.0]
    d.start_rot[:] = [1.0, 0.0, 0.0, 0.0]
    table = torch.empty(T, 3 + 3 * J, dtype=torch.float64, device=DEV)
    rc = ops.lib().zeggs_pose_to_bvh_table(C.byref(d), C.c_void_p(rpos.data_ptr()), C.c_void_p(rrot.data_ptr()),
                                           C.c_void_p(lpos.data_ptr()), C.c_void_p(ltxy.data_ptr()), C.c_void_p(rpos.data_ptr()),
                                           C.c_void_p(rrot.data_ptr()), C.c_void_p(seq_dev.data_ptr()), C.c_void_p(table.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return table, (rpos, rrot, lpos, ltxy)


def test_the_real_case_a_pose_to_bvh_table():
    table, _ = _rollout_table()
    want, ends = host_text(table.cpu().numpy())
    before = anim.TEXT_FALLBACKS
    got = anim.format_rows_device(table)
    assert bytes(got[0]) == want and anim.TEXT_FALLBACKS == before
    _, row_end, status, rc = raw_call(table, table.shape[0] * (table.shape[1] * 24 + 1))
    assert rc == 0 and status == 0 and np.array_equal(row_end, ends)


@pytest.mark.parametrize("emit", [0, 1])
@pytest.mark.parametrize("rows,cols", [(7, 65), (5, 1027), (33, 228)])
def test_canary_and_exact_cap(rows, cols, emit):
    """64 guard bytes on either side of the text stay intact, with the documented bound as cap and with cap = row_end[-1] exactly;
    one byte less leaves the last row out, says so in status bit 1 and still writes nothing outside"""
    table = mixed_table(rows, cols, seed=77 + rows)
    want, ends = host_text(table)
    dev = torch.as_tensor(table, device=DEV)
    ops.set_option("text_emit", emit)
    try:
        for cap in (rows * (cols * 24 + 1), len(want)):
            buf, row_end, status, rc = raw_call(dev, cap, guard=64)
            assert rc == 0 and status == 0
            assert (buf[:64] == 0xA5).all() and (buf[64 + len(want):] == 0xA5).all(), cap
            assert buf[64:64 + len(want)].tobytes() == want and np.array_equal(row_end, ends)
        buf, row_end, status, rc = raw_call(dev, len(want) - 1, guard=64)
        keep = int(ends[-2]) if rows > 1 else 0
        assert rc == 0 and status == 2 and np.array_equal(row_end, ends)
        assert (buf[:64] == 0xA5).all() and (buf[64 + keep:] == 0xA5).all() and buf[64:64 + keep].tobytes() == want[:keep]
    finally:
        ops.set_option("text_emit", 0)


def test_out_of_domain_goes_to_the_host_formatter():
    table = mixed_table(4, 5, seed=9)
    clean = torch.as_tensor(table, device=DEV)
    table[0, 1], table[2, 4], table[3, 0] = np.nan, np.inf, 1e300
    dirty = torch.as_tensor(table, device=DEV)
    buf, row_end, status, rc = raw_call(dirty, 4 * (5 * 24 + 1), guard=64)
    assert rc == 0 and status & 1
    assert (buf[:64] == 0xA5).all() and (buf[64 + int(row_end[-1]):] == 0xA5).all()
    placeholder = table.copy()
    placeholder[0, 1] = placeholder[2, 4] = placeholder[3, 0] = 0.0
    assert buf[64:64 + int(row_end[-1])].tobytes() == anim.format_rows(placeholder)      # "0.000000" in the three slots
    before = anim.TEXT_FALLBACKS
    got = anim.format_rows_device(dirty, cuts=[1])
    assert anim.TEXT_FALLBACKS == before + 1
    want = anim.format_rows(table, any_magnitude=True)       # (the host's snprintf: "nan", "inf" and the 301 digits of 1e300)
    assert b"".join(bytes(p) for p in got) == want and bytes(got[0]) == anim.format_rows(table[:1])
    assert len(want.split()[15]) == 308
    assert b"nan" in bytes(got[0]) and b"inf" in bytes(got[1])
    anim.format_rows_device(clean)
    assert anim.TEXT_FALLBACKS == before + 1


def test_cuts():
    table = mixed_table(300, 11, seed=5)
    want, ends = host_text(table)
    cuts = [0, 1, 1, 17, 256, 299]
    got = anim.format_rows_device(torch.as_tensor(table, device=DEV), cuts=cuts)
    assert len(got) == len(cuts) + 1 and b"".join(bytes(p) for p in got) == want
    starts = np.concatenate([[0], ends])
    pos = 0
    for piece, row in zip(got, [0] + cuts):
        assert pos == starts[row]                                                        # every piece starts at a row start
        pos += len(bytes(piece))
    assert bytes(got[4]) == anim.format_rows(table[17:256])


def test_writers_device_and_host_give_identical_files(tmp_path, monkeypatch):
    """write_bvh_channels / write_bvh / bvh_save on a small synthetic skeleton, 50 frames: text = "device", text = "host" and the module
    default write the same bytes; a host table takes the device from TEXT_UPLOAD_MIN_NUMBERS numbers on (the threshold is moved to
    either side of this table's size)"""
    table, (rpos, rrot, lpos, ltxy) = _rollout_table(50)
    ch = anim.bvh_channels(rpos, rrot, lpos, ltxy, np.array([0, 0, 0]), np.array([1, 0, 0, 0]))
    kw = dict(parents=synth.PARENTS, names=synth.BONE_NAMES, order="zyx", dt=synth.DT)
    calls = []
    orig = anim.format_rows_device
    monkeypatch.setattr(anim, "format_rows_device", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    anim.write_bvh_channels(str(tmp_path / "h.bvh"), *ch, text="host", **kw)
    assert calls == []
    anim.write_bvh_channels(str(tmp_path / "d.bvh"), *ch, text="device", **kw)
    anim.write_bvh_channels(str(tmp_path / "default.bvh"), *ch, **kw)
    assert anim.TEXT == "device" and calls == [1, 1]
    anim.write_bvh(str(tmp_path / "w.bvh"), rpos, rrot, lpos, ltxy, synth.PARENTS, synth.BONE_NAMES, "zyx", synth.DT,
                   np.array([0, 0, 0]), np.array([1, 0, 0, 0]), text="device")
    want = (tmp_path / "h.bvh").read_bytes()
    assert want.count(b"\n") > 50
    for name in ("d", "default", "w"):
        assert (tmp_path / f"{name}.bvh").read_bytes() == want, name
    # bvh_save on HOST arrays: below the threshold the host formats, from it on the device does -- same file
    data = dict(order="zyx", offsets=ch[0][0].cpu().numpy(), names=synth.BONE_NAMES, frametime=synth.DT, parents=synth.PARENTS,
                positions=ch[0].cpu().numpy(), rotations=ch[1].cpu().numpy())
    numbers = 50 * table.shape[1]
    del calls[:]
    monkeypatch.setattr(anim, "TEXT_UPLOAD_MIN_NUMBERS", numbers + 1)
    anim.bvh_save(tmp_path / "s_small.bvh", data)
    assert calls == []
    monkeypatch.setattr(anim, "TEXT_UPLOAD_MIN_NUMBERS", numbers)
    anim.bvh_save(tmp_path / "s_large.bvh", data)
    assert calls == [1]
    with pytest.raises(ValueError):
        anim.bvh_save(tmp_path / "x.bvh", data, text="gpu")
    assert (tmp_path / "s_small.bvh").read_bytes() == want and (tmp_path / "s_large.bvh").read_bytes() == want


def _generate_fixture(golden_dir, tmp_path):
    import scipy.io.wavfile as wavfile
    gd = np.load(golden_dir / "generate.npz")
    net, data = tmp_path / "net", tmp_path / "data"
    net.mkdir(), data.mkdir()
    se, de, st = helpers.build_nets()
    torch.save(se, net / "speech_encoder.pt"), torch.save(de, net / "decoder.pt"), torch.save(st, net / "style_encoder.pt")
    np.savez(data / "stats.npz", **synth.make_stats())
    json.dump(synth.data_definition(), open(data / "data_definition.json", "w"))
    conf = dict(audio_conf=dict(pre_emphasis=False, pre_emph_coeff=0.97, centered=True, real_amplitude=True,
                                normalize_mel_bins=True, normalize_range=True, min_clipping=1e-5, sampling_rate=16000,
                                mel_fmin=20, mel_fmax=7600, n_mel_channels=80, filter_length=800, hop_length=200,
                                resample_method="linear", normalize_loudness=False),
                audio_feature_type=["mel_spec", "energy"])
    json.dump(conf, open(data / "data_pipeline_conf.json", "w"))
    ex = tmp_path / "ex.bvh"
    ex.write_bytes(gd["exemplar_bvh"].tobytes())
    return net, data, ex, wavfile


def _record_tables(monkeypatch):
    """every table the writers hand to their text staging, as host arrays with the spans it is cut at"""
    rec = []
    orig = generate._TextStaging.submit

    def submit(self, table, spans, block):
        rec.append((table.cpu().numpy().copy(), list(spans)))
        return orig(self, table, spans, block)
    monkeypatch.setattr(generate._TextStaging, "submit", submit)
    return rec


def _split(bvh):
    """BVH bytes -> (everything up to and including the "Frame Time" line, frame count, the motion rows)"""
    head, motion = bvh.split(b"MOTION\n")
    l1, l2, body = motion.split(b"\n", 2)
    assert l1.startswith(b"Frames: ") and l2.startswith(b"Frame Time: ")
    return head + l1 + l2, int(l1.split()[1]), body


def test_generate_gestures_device_text_equals_host_text(golden_dir, tmp_path, monkeypatch):
    """three short jobs of different lengths on two rows in chunks of 8 frames (rows of one table change clips at chunk boundaries;
    every chunk's table is cut into the clips' pieces), under anim.TEXT = "device" and again under "host".  Two decodes of the same
    job differ in the last digits (the split-K atomics of the prologue products: a row read 167.192859 in one run and 167.192861 in
    the next), so the files of the two runs are not compared with each other: in EACH run every table that reaches the text
    staging is recorded, and every file must be, byte for byte, its header + the host formatter's text of exactly those rows in
    the slot plan's order.  Headers and frame counts are equal across the runs, the device formatter ran, nothing fell back."""
    net, data, ex, wavfile = _generate_fixture(golden_dir, tmp_path)
    jobs = []
    for tag, samples, seed in (("a", 16000 * 1 + 300, 3), ("b", 11000, 4), ("c", 6000, 5)):
        wavfile.write(tmp_path / f"{tag}.wav", 16000, synth.synth_wav(samples, seed=seed))
        jobs.append(generate.Job(tmp_path / f"{tag}.wav", [(ex, None)], file_name=tag, first_pose=ex, temperature=1e8, seed=seed,
                                 blend_type="add", blend_ratio=[1.0]))
    calls = []
    orig = anim.table_text_device
    monkeypatch.setattr(anim, "table_text_device", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    rec = _record_tables(monkeypatch)
    before = anim.TEXT_FALLBACKS
    heads = {}
    for mode in ("device", "host"):
        monkeypatch.setattr(anim, "TEXT", mode)
        del calls[:], rec[:]
        generate.generate_gestures(jobs, net, data, tmp_path / mode, style_encoding_type="example", batch=2, chunk=8)
        assert ops.batch_last_path() == "persistent"
        assert len(calls) == (len(rec) if mode == "device" else 0) and len(rec) > 3, (mode, len(calls), len(rec))
        files = [_split((tmp_path / mode / f"{j.file_name}.bvh").read_bytes()) for j in jobs]
        lengths = [f[1] for f in files]
        assert len(set(lengths)) == 3, lengths
        plan = generate.plan_slots(lengths, 2, 8)
        assert len(plan) == len(rec)
        assert any(len({j for _, j, _, _ in pieces}) == 2 for pieces in plan)            # a table shared by two clips
        assert any(k == 0 for pieces in plan[1:] for _, _, k, _ in pieces)               # a row changes clips at a chunk boundary
        want = [[] for _ in jobs]
        for pieces, (table, spans) in zip(plan, rec):
            live = [(j, n + (1 if k == 0 else 0)) for _, j, k, n in pieces if n + (1 if k == 0 else 0) > 0]
            assert [n for _, n in live] == [n for _, n in spans] and table.shape[0] == sum(n for _, n in spans)
            for (j, n), (s0, _) in zip(live, spans):
                want[j].append(anim.format_rows(table[s0:s0 + n]))
        for j, (head, _, body) in enumerate(files):
            assert body == b"".join(want[j]), (mode, jobs[j].file_name)
        heads[mode] = [(f[0], f[1]) for f in files]
    assert heads["device"] == heads["host"] and anim.TEXT_FALLBACKS == before


def test_streaming_writer_device_text_equals_host_text(golden_dir, tmp_path, monkeypatch):
    """generate._decode_to_bvh_streaming with a small chunk (several chunks and the short tail chunk), under both settings: the file
    is its header + the host formatter's text of the very tables the run produced (see the test above for why the two runs are
    not compared with each other); same header and frame count under both"""
    net, data, ex, wavfile = _generate_fixture(golden_dir, tmp_path)
    wavfile.write(tmp_path / "a.wav", 16000, synth.synth_wav(16000 * 2 + 777, seed=31))          # 2 s -> 120-odd frames
    monkeypatch.setattr(generate, "STREAM_MIN_FRAMES", 20)
    monkeypatch.setattr(generate, "STREAM_CHUNK", 37)
    monkeypatch.setattr(generate, "STREAM_BLOCK", 16)
    streamed = []
    orig = generate._decode_to_bvh_streaming
    monkeypatch.setattr(generate, "_decode_to_bvh_streaming", lambda *a, **k: (streamed.append(1), orig(*a, **k))[1])
    rec = _record_tables(monkeypatch)
    kw = dict(style_encoding_type="example", blend_type="add", blend_ratio=[1.0], first_pose=ex, temperature=1e8, seed=1234)
    before = anim.TEXT_FALLBACKS
    heads = {}
    for mode in ("device", "host"):
        monkeypatch.setattr(anim, "TEXT", mode)
        del rec[:]
        generate.generate_gesture(tmp_path / "a.wav", [(ex, None)], net, data, tmp_path / "res", file_name=mode, **kw)
        head, frames, body = _split((tmp_path / "res" / f"{mode}.bvh").read_bytes())
        rows = [t.shape[0] for t, _ in rec]
        assert len(rows) >= 4 and sum(rows) == frames and rows[-1] < rows[1], rows       # several chunks and a short tail chunk
        assert body == b"".join(anim.format_rows(t) for t, _ in rec), mode
        heads[mode] = (head, frames)
    assert streamed == [1, 1] and anim.TEXT_FALLBACKS == before and heads["device"] == heads["host"]
