"""Feet that stay planted (include/zeggs_hip_plant.h): zeggs_live_plant against the float64 oracle (tests/live_plant_oracle.py) on
ALL frames and chains (tests/test_live_plant_cpu.py asserts the margins that allow it), its independence of the cuts and of the
other rows bit for bit, thresholds that never plant, the server's "frames" and "contacts" from step() to close() on the plain, the
re-timed and the filtered head, a snapshot taken while a foot is held, a server without the stage, and generate_gesture(plant=)."""
import numpy as np
import pytest
import torch

import live_plant_oracle as po
import test_gpu_live_frames as plain
import test_gpu_live_push as lp
import test_gpu_live_refilter as filtered
import test_gpu_live_retime as unfiltered
from zeggs import anim, audio, capi, generate, live, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23            # the head's bound, for the same reason: a float64 value rounded to float32 once (2^-24) plus float64 noise
GUARD = 7.25
ROWS = 2
SEEDS = (1, 2)              # the two rows of a call


def _dev(c):
    return tuple(torch.as_tensor(np.array(c[k]), device=DEV) for k in ("pose", "rpos", "rrot"))


def _stage(c, rows=ROWS, max_frames=po.T_WALK, opt=None):
    conf = ops.plant_options(po.plant_kwargs(opt or c["opt"], c["chains"]), c["parents"], c["names"])
    return ops.LivePlant(rows, c["parents"], max_frames, conf, (opt or c["opt"])["dt"], DEV)


class _Out:
    """the destinations of one record with a guard behind each"""

    def __init__(self, lp_, count):
        self.count, self.PO, self.C = count, lp_.pose_floats, lp_.C
        self.pose = torch.full((count * self.PO + 8,), GUARD, device=DEV)
        self.flags = torch.full((count * self.C + 8,), 77, device=DEV, dtype=torch.uint8)

    def guards_ok(self):
        return bool((self.pose[self.count * self.PO:] == GUARD).all() and (self.flags[self.count * self.C:] == 77).all())

    def host(self):
        return (self.pose[:self.count * self.PO].cpu().numpy().reshape(self.count, self.PO),
                self.flags[:self.count * self.C].cpu().numpy().reshape(self.count, self.C))


def _record(q, row, src, a, c, out):
    pose, rpos, rrot = src
    q.pose, q.rpos, q.rrot = pose[a:].data_ptr(), rpos[a:].data_ptr(), rrot[a:].data_ptr()
    q.pose_ld, q.rpos_ld, q.rrot_ld, q.out_ld = pose.stride(0), rpos.stride(0), rrot.stride(0), out.PO
    q.out, q.contacts, q.row, q.count = out.pose.data_ptr(), out.flags.data_ptr(), row, c


def _run_cuts(st, row, src, cuts):
    """frames [0, sum(cuts)) of `src` through row `row` in calls of cuts[i] frames each (one record, in the kernel arguments) ->
    (rows, flags) concatenated; every guard is looked at"""
    rows, flags, a = [], [], 0
    rec = (capi.PlantRow * 1)()
    for c in cuts:
        out = _Out(st, c)
        _record(rec[0], row, src, a, c, out)
        ops.live_plant(st, rec, 1)
        assert out.guards_ok(), (a, c)
        r, f = out.host()
        rows.append(r), flags.append(f)
        a += c
    return np.concatenate(rows), np.concatenate(flags)


def _run_together(st, srcs, T):
    """rows 0 .. of `st` in ONE launch, T frames each, the records on the device -> [(rows, flags)]"""
    n = len(srcs)
    recs, outs = (capi.PlantRow * n)(), [_Out(st, T) for _ in srcs]
    for r, (src, out) in enumerate(zip(srcs, outs)):
        _record(recs[r], r, src, 0, T, out)
    dev = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)
    ops.live_plant(st, recs, n, dev.data_ptr())
    assert all(o.guards_ok() for o in outs)
    return [o.host() for o in outs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _compare(c, got, flags, T):
    """the bounds of the issue on the first T frames: the corrected ltxy of u, m, e within 2^-23 of the oracle's float64 value,
    every other float the input's bits, the contact flags exactly the oracle's -- on ALL frames and chains"""
    J, det = len(c["parents"]), c["det"]
    assert np.array_equal(flags, c["contacts"][:T]), "contact flags"
    want_xy, got_xy, in_xy = po.split(c["out"][:T], J)[1], po.split(got, J)[1], po.split(c["pose"][:T], J)[1]
    mine = np.zeros((T, J), bool)
    worst = 0.0
    for f in range(T):
        for ch, chain in enumerate(c["idx"]):
            for k, j in enumerate(chain):
                if det["solved"][f, ch]:
                    mine[f, j] = True
                    e = np.abs(got_xy[f, j].reshape(6).astype(np.float64) - po.to_xy(det["lrot"][f, ch, k])).max()
                    worst = max(worst, e)
                    assert e <= EPS, (f, ch, j, e)
                    assert np.abs(got_xy[f, j].astype(np.float64) - want_xy[f, j]).max() <= EPS
    other = got.copy()
    po.split(other, J)[1][mine] = in_xy[mine]
    assert np.array_equal(_bits(other), _bits(c["pose"][:T])), "a float outside the solved chains changed"
    return worst


# ----------------------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("T", [1, 2, 7, 40])
@pytest.mark.parametrize("name", ["walker", "rig"])
def test_kernel_equals_the_oracle(name, T):
    """2 rows (two seeds of the scripted walk) in one launch, the first T frames, both skeletons: every frame and chain compared"""
    cases = [po.case(name, s) for s in SEEDS]
    st = _stage(cases[0])
    for r in range(ROWS):
        ops.live_plant_reset(st, r)
    got = _run_together(st, [tuple(t[:T] for t in _dev(c)) for c in cases], T)
    for c, (rows, flags) in zip(cases, got):
        worst = _compare(c, rows, flags, T)
        print(f"{name} T={T}: worst ltxy error {worst / EPS:.3f} of 2^-23; {int(c['det']['solved'][:T].sum())} solves, {int(flags.sum())} contacts")
    if T == 40:
        assert all(f.any() and not f.all() for _, f in got)


# ----------------------------------------------------------------------------- 2. cuts and company
@pytest.mark.parametrize("name", ["walker", "rig"])
def test_cuts_and_company_do_not_change_a_bit(name):
    """(40), 1 x 40, (3, 17, 20), (7, 1, 32) give the same bytes and leave the same state; a row alone and the row sharing the
    call give the same bytes; a row that is absent from a call keeps its state"""
    cases = [po.case(name, s) for s in SEEDS]
    srcs = [_dev(c) for c in cases]
    st = _stage(cases[0], rows=3)
    ref = None
    for cuts in ((40,), (1,) * 40, (3, 17, 20), (7, 1, 32)):
        ops.live_plant_reset(st, 1)
        rows, flags = _run_cuts(st, 1, srcs[0], cuts)
        torch.cuda.synchronize()
        state = st.state.cpu().numpy().copy()
        if ref is None:
            ref = (rows, flags, state)
            _compare(cases[0], rows, flags, 40)
        assert np.array_equal(_bits(rows), _bits(ref[0])) and np.array_equal(flags, ref[1]) and np.array_equal(state, ref[2]), cuts
    spans = [ops.live_plant_spans(st, r)[0] for r in range(3)]
    assert not ref[2][spans[0][0]:spans[0][0] + spans[0][1]].any() and not ref[2][spans[2][0]:].any()      # rows 0 and 2 were never touched
    both = _stage(cases[0], rows=2)
    for r in range(2):
        ops.live_plant_reset(both, r)
    together = _run_together(both, srcs, 40)
    for r, c in enumerate(cases):
        alone = _stage(c, rows=1)
        ops.live_plant_reset(alone, 0)
        rows, flags = _run_cuts(alone, 0, srcs[r], (40,))
        assert np.array_equal(_bits(rows), _bits(together[r][0])) and np.array_equal(flags, together[r][1]), r
    # anim.plant_feet is the same launch on a fresh one-row state
    c = cases[0]
    out, flags = anim.plant_feet(*srcs[0], c["parents"], c["names"], c["opt"]["dt"], **po.plant_kwargs(c["opt"], c["chains"]))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref[0])) and np.array_equal(flags.cpu().numpy(), ref[1])
    # ... and carried on from piece to piece with a stage
    stage = anim.plant_stage(c["parents"], c["names"], c["opt"]["dt"], DEV, max_frames=16, **po.plant_kwargs(c["opt"], c["chains"]))
    pieces = [anim.plant_feet(*(t[a:b] for t in srcs[0]), c["parents"], c["names"], c["opt"]["dt"], stage=stage) for a, b in ((0, 23), (23, 24), (24, 40))]
    assert np.array_equal(_bits(torch.cat([p[0] for p in pieces]).cpu().numpy()), _bits(ref[0]))


def test_thresholds_that_never_plant_return_the_input():
    """a speed and a height no frame meets: the output bytes are the input bytes, no contact"""
    for name in ("walker", "rig"):
        c = po.case(name, 1)
        never = po.options(speed=(0.0, 0.0), height=(-1e9, -1e9))
        st = _stage(c, rows=1, opt=never)
        ops.live_plant_reset(st, 0)
        rows, flags = _run_cuts(st, 0, _dev(c), (40,))
        assert np.array_equal(_bits(rows), _bits(c["pose"])) and not flags.any()


# ----------------------------------------------------------------------------- 3. the server
FRAMES = dict(plain.FRAMES, text=True)
NSAMP = 16000                    # 1 s: 60 frames
# thresholds a random network's motion meets now and then, so that feet do plant and do come off again
LOOSE = dict(chains="auto", speed=(60.0, 120.0), height=(1e6, 2e6), ground=0.0, slack=3.0, release=5, stretch=0.999)
ALL = ("local", "world", "bvh")


def _head_again(kind, w, place, ratio):
    """the head of the server's form on a fresh state, records of 20 frames, over the rows w = (pose, rpos, rrot) on the device"""
    T = w[0].shape[0]
    cuts = [20] * (T // 20) + ([T % 20] if T % 20 else [])
    if kind == "plain":
        lf = ops.LiveFrames(1, synth.PARENTS, 20, ALL, "zyx", None, DEV)
        plain._reset(lf, 0, w, place)
        return plain._run_cuts(lf, 0, w, cuts)
    if kind == "retimed":
        lt = ops.LiveRetime(1, synth.PARENTS, 20, ALL, "zyx", None, DEV)
        unfiltered._reset(lt, 0, w, place)
        return unfiltered._run_cuts(lt, 0, w, cuts, ratio)
    lr = ops.LiveRefilter(1, synth.PARENTS, 20, 10, None, ALL, "zyx", None, DEV)
    filtered._reset(lr, 0, w, place)
    return filtered._run_cuts(lr, 0, w, cuts, ratio)


@pytest.mark.parametrize("kind", ["plain", "retimed", "filtered"])
def test_server_frames_are_the_head_of_the_planted_rows(kind):
    """two streams on a planting server of 2 rows at tick 4 (one placed), on the plain head, the re-timed head (frame_rate=30) and
    the filtered head (frame_rate=30): the raw "pose", "rpos", "rrot" of a stream collected over step() ... close(), through
    anim.plant_feet as a whole and then through the head with a fresh state, equal the server's "frames" bit for bit, and the flags
    the server's "contacts" -- the flags of the MODEL frames, also where the stream's own frames are fewer.  The thresholds are
    permissive: contacts happen and the planted rows differ from the raw ones.  One more launch a step than without the stage."""
    retime = dict(plain={}, retimed=dict(retime=dict(max_rate=60)), filtered=dict(retime=dict(max_rate=60, filter=True, min_rate=24)))[kind]
    srv = lp._server(2, 4, frames=FRAMES, plant=LOOSE, **retime)
    base = lp._server(2, 4, frames=FRAMES, **retime)
    rate = None if kind == "plain" else 30
    places = [None, plain.fo.PLACE]
    sids = [srv.open(lp._first(3 + r), lp._style(70 + r), **({} if rate is None else dict(frame_rate=rate)),
                     **({} if p is None else dict(start_position=p[0], start_rotation=p[1]))) for r, p in enumerate(places)]
    wavs = {sid: lp._wav(NSAMP - 1600 * r, 60 + r) for r, sid in enumerate(sids)}
    parts = plain._serve(srv, wavs, 1600, True)
    bsids = [base.open(lp._first(3), lp._style(70), **({} if rate is None else dict(frame_rate=rate))) for _ in range(2)]
    plain._serve(base, {sid: lp._wav(NSAMP, 60) for sid in bsids}, 1600, True)
    assert srv.stats["launches_per_step"] == base.stats["launches_per_step"] + 1
    for r, sid in enumerate(sids):
        live_parts = [p for p in parts[sid] if p]
        assert all("contacts" in p and p["contacts"].shape == (p["pose"].shape[0], 2) and p["contacts"].dtype == bool for p in live_parts)
        w = unfiltered._whole(parts[sid])
        contacts = np.concatenate([p["contacts"] for p in live_parts])
        T = audio.n_anim_frames(wavs[sid].size)
        assert w["pose"].shape[0] == T == contacts.shape[0]
        src = tuple(torch.as_tensor(w[k], device=DEV) for k in lp.KEYS)
        planted, flags = anim.plant_feet(*src, synth.PARENTS, synth.BONE_NAMES, synth.DT, **LOOSE)
        assert np.array_equal(flags.cpu().numpy().astype(bool), contacts)
        assert contacts.any() and not np.array_equal(_bits(planted.cpu().numpy()), _bits(w["pose"]))
        again = _head_again(kind, (planted, src[1], src[2]), places[r], (1, 2))
        unfiltered._same_bits(w["frames"], again, (kind, r))
        raw = _head_again(kind, src, places[r], (1, 2))
        assert raw["bvh"].tobytes() != again["bvh"].tobytes()
        print(f"{kind} stream {r}: {T} frames, {int(contacts.sum())} contact flags, {w['frames']['bvh'].shape[0]} frames out")


def test_a_snapshot_taken_while_a_foot_is_held_goes_on_bit_for_bit():
    """a stream on a planting server, a snapshot at a step after which a chain is HELD (read from the chain's state), restored into
    another row of the same server and into a second server: with the same audio the three hand out the same "frames" and
    "contacts" bit for bit wherever their raw rows are the same bits; restore followed by snapshot gives the blob; the blob has
    the planting fields in its fingerprint and the chains' states behind the head's pieces, and neither kind of server takes the
    other's blobs"""
    A, B, P = lp._server(3, 4, frames=FRAMES, plant=LOOSE), lp._server(2, 4, frames=FRAMES, plant=LOOSE), lp._server(2, 4, frames=FRAMES)
    wav = lp._wav(NSAMP, 61)
    sid = A.open(lp._first(3), lp._style(71))
    parts, i, held = [], 0, False
    while not held and i < 6:
        A.push(sid, wav[1600 * i:1600 * (i + 1)])
        parts.append(A.step().get(sid))
        i += 1
        if parts[-1]:
            held = bool(parts[-1]["contacts"][-1].any())
    assert held, "no chain is held at the end of any of the first steps"
    off, nb = ops.live_plant_spans(A._pl, 0)[0]
    torch.cuda.synchronize()
    modes = A._pl.state[off:off + nb].cpu().numpy().view(np.int32).reshape(4, 22)[:2, 18]
    assert modes.any()
    blob = A.snapshot(sid)
    info = live.snapshot_info(blob)
    assert len(info["fingerprint"]) == 43 + len(live.SNAP_FINGERPRINT_PLANT) and info["fingerprint"]["plant_slack"] == LOOSE["slack"]
    head_plain = live.snapshot_info(P.snapshot(P.open(lp._first(3), lp._style(71))))
    assert info["sections"]["head"][1] == live._a16(head_plain["sections"]["head"][1]) + 4 * 88 and len(head_plain["fingerprint"]) == 43
    twin, far = A.restore(blob), B.restore(blob)
    pay = lambda b: (lambda x: (x.__setitem__(slice(16, 24), 0), x.tobytes())[1])(np.array(b))  # noqa: E731
    assert pay(A.snapshot(twin)) == pay(blob) and pay(B.snapshot(far)) == pay(blob)
    with pytest.raises(ValueError, match="taken from a server with plant, this one has none"):
        P.restore(blob)
    with pytest.raises(ValueError, match="taken from a server without plant"):
        A.restore(P.snapshot(0))
    halves = {(A, sid): [], (A, twin): [], (B, far): []}
    for j in range(i, 10):
        for (srv, s) in halves:
            srv.push(s, wav[1600 * j:1600 * (j + 1)])
        for srv in (A, B):
            while True:
                out = srv.step()
                if not out:
                    break
                for (s2, s), got in halves.items():
                    if s2 is srv and s in out:
                        got.append(out[s])
    for (srv, s), got in halves.items():
        got.append(srv.close(s))
    src = halves[(A, sid)]
    for key, got in halves.items():
        assert len(got) == len(src)
        if key == (A, sid):
            continue
        for a, b in zip(src, got):
            if all(torch.equal(a[k], b[k]) for k in lp.KEYS):
                assert np.array_equal(a["contacts"], b["contacts"])
                unfiltered._same_bits(a["frames"], b["frames"], key)
        # whatever the decoder's sums did: a fork's frames are the head of plant_feet of ITS rows, continued from the snapshot
    whole = unfiltered._whole([p for p in parts if p] + halves[(A, twin)])
    rows = tuple(torch.as_tensor(whole[k], device=DEV) for k in lp.KEYS)
    planted, flags = anim.plant_feet(*rows, synth.PARENTS, synth.BONE_NAMES, synth.DT, **LOOSE)
    again = _head_again("plain", (planted, rows[1], rows[2]), None, (1, 1))
    unfiltered._same_bits(whole["frames"], again, "the fork, whole")
    assert np.array_equal(flags.cpu().numpy().astype(bool), np.concatenate([p["contacts"] for p in parts if p] + [p["contacts"] for p in halves[(A, twin)] if p]))


@pytest.mark.parametrize("rows", [1, 2])
def test_a_server_without_plant_is_the_server_it_was(rows):
    """LiveServer(frames=...) without `plant`: no planting state, no scratch rows, the staging block of the head's size, no
    "contacts", and the launches per step of the head alone (10 + 2 at one row, 9 + 2 otherwise); with `plant`: one more"""
    srv = lp._server(rows, 4, frames=plain.FRAMES)
    assert srv._pl is None and srv._pl_pose is None and srv.plant_conf is None and not hasattr(srv._fr_stage, "tail_recs")
    J = len(synth.PARENTS)
    assert srv._fr_stage.nbytes == live.frames_block_bytes(rows * srv._fr.d.max_frames, J, 7)
    assert srv._fr.state.numel() == capi.api().zeggs_live_frames_state_bytes(srv._fr.d)
    sids = [srv.open(lp._first(3), lp._style(70 + r)) for r in range(rows)]
    parts = plain._serve(srv, {sid: lp._wav(NSAMP // 2, 60 + r) for r, sid in enumerate(sids)}, 1600, rows > 1)
    assert srv.stats["launches_per_step"] == (12 if rows == 1 else 11)
    assert all("contacts" not in p for v in parts.values() for p in v if p)
    fp = srv._fingerprint()
    assert set(fp) == set(live.SNAP_FINGERPRINT)
    planting = lp._server(rows, 4, frames=plain.FRAMES, plant=LOOSE)
    assert planting._fr_stage.nbytes == srv._fr_stage.nbytes + rows * srv._fr.d.max_frames * 2
    psids = [planting.open(lp._first(3), lp._style(70 + r)) for r in range(rows)]
    plain._serve(planting, {sid: lp._wav(NSAMP // 2, 60 + r) for r, sid in enumerate(psids)}, 1600, rows > 1)
    assert planting.stats["launches_per_step"] == (13 if rows == 1 else 12)
    assert set(planting._fingerprint()) == set(live.SNAP_FINGERPRINT) | set(live.SNAP_FINGERPRINT_PLANT)


# ----------------------------------------------------------------------------- 4. generate_gesture(plant=...)
@pytest.mark.parametrize("path", ["one-launch", "chunked"])
def test_generate_gesture_writes_the_planted_clip(path, golden_dir, tmp_path, monkeypatch):
    """a 64-frame clip through generate_gesture(plant=...): the BVH written equals anim.plant_feet of the decoded rows, whole and on
    a fresh state, through the same writer -- on the one-launch path and on the chunked long-clip path (chunks of 23 frames: the
    contact state is carried from chunk to chunk); feet do plant, and the file differs from the one without `plant`"""
    import test_gpu_text as gt
    net, data, ex, wavfile = gt._generate_fixture(golden_dir, tmp_path)
    wavfile.write(tmp_path / "a.wav", 16000, synth.synth_wav(17067, seed=31))          # 64 frames
    if path == "chunked":
        monkeypatch.setattr(generate, "STREAM_MIN_FRAMES", 20)
        monkeypatch.setattr(generate, "STREAM_CHUNK", 23)
        monkeypatch.setattr(generate, "STREAM_BLOCK", 16)
    seen = []
    orig = anim.plant_feet
    monkeypatch.setattr(anim, "plant_feet", lambda pose, rpos, rrot, *a, **k: (seen.append((pose.clone(), rpos.clone(), rrot.clone())), orig(pose, rpos, rrot, *a, **k))[1])
    kw = dict(style_encoding_type="example", blend_type="add", blend_ratio=[1.0], first_pose=ex, temperature=1e8, seed=1234)
    generate.generate_gesture(tmp_path / "a.wav", [(ex, None)], net, data, tmp_path / "res", file_name="planted", plant=LOOSE, **kw)
    calls = len(seen)
    assert calls == (1 if path == "one-launch" else 4), calls
    generate.generate_gesture(tmp_path / "a.wav", [(ex, None)], net, data, tmp_path / "res", file_name="raw", **kw)
    assert len(seen) == calls
    monkeypatch.setattr(anim, "plant_feet", orig)
    pose, rpos, rrot = (torch.cat([s[i] for s in seen]) for i in range(3))
    T, J = pose.shape[0], len(synth.PARENTS)
    assert T == 64
    planted, flags = anim.plant_feet(pose, rpos, rrot, synth.PARENTS, synth.BONE_NAMES, synth.DT, **LOOSE)
    assert bool(flags.any()) and not torch.equal(planted, pose)
    anim.write_bvh(str(tmp_path / "want.bvh"), rpos, rrot, planted[:, 6:6 + 3 * J].reshape(T, J, 3), planted[:, 6 + 3 * J:6 + 9 * J].reshape(T, J, 2, 3),
                   synth.PARENTS, synth.BONE_NAMES, "zyx", synth.DT, np.array([0, 0, 0]), np.array([1, 0, 0, 0]))
    got, want, raw = ((tmp_path / p).read_bytes() for p in ("res/planted.bvh", "want.bvh", "res/raw.bvh"))
    assert got == want and got != raw and got.count(b"\n") == raw.count(b"\n")
    with pytest.raises(ValueError, match="plant: .*no joint named 'Tail'"):
        generate.generate_gesture(tmp_path / "a.wav", [(ex, None)], net, data, tmp_path / "res", plant=dict(chains=[("Hips", "Spine", "Tail")]), **kw)
