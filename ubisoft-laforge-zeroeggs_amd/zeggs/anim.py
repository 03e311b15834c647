"""Animation plumbing around the decoder: BVH file I/O on the host, feature extraction, BVH-channel conversion (csrc/anim.hip,
float64) and the formatting of the motion text (csrc/text.hip) on the device.

Semantics follow the reference so that `generate_gesture()` consumes and produces the same files:
  ZEGGS/anim/bvh.py (BVH reader/writer), ZEGGS/data_pipeline.py:90-228 (preprocess_animation),
  ZEGGS/generate.py:389 + ZEGGS/utils.py:47-87 (two-axis rotations -> quaternions -> euler channels, write_bvh).
The NumPy restatement of the device kernels lives in oracle/anim.py (test infrastructure).
"""
import ctypes as C
import re

import numpy as np
import torch

from . import ops
from .capi import ANIM_OUT_FIELDS, AnimDims, AnimOut, BvhDims, api  # noqa: F401

_CHAN = {"Xrotation": "x", "Yrotation": "y", "Zrotation": "z"}
_CHAN_INV = {v: k for k, v in _CHAN.items()}


# ----------------------------------------------------------------------------- BVH
def bvh_load(filename):
    """-> dict(rotations [F,J,3] degrees, positions [F,J,3], offsets [J,3], parents [J], names, order, frametime)"""
    names, offsets, parents, chans = [], [], [], []
    stack, order, end_site = [], None, False
    with open(filename, "rb") as f:
        raw = f.read()
    # the MOTION section starts at a line that holds nothing but the keyword (a joint called LOCOMOTION_root is not it: ADVICE r4)
    msec = re.search(rb"(?m)^[ \t]*MOTION[ \t]*\r?$", raw)
    if msec is None:
        raise ValueError(f"{filename}: no MOTION section (a line holding only the keyword MOTION)")
    mpos, mend = msec.start(), msec.end()
    lines = iter(raw[:mpos].decode().splitlines() + ["MOTION"])
    for line in lines:
        tok = line.split()
        if not tok:
            continue
        if tok[0] in ("ROOT", "JOINT"):
            names.append(tok[1])
            offsets.append([0.0, 0.0, 0.0])
            parents.append(stack[-1] if stack else -1)
            chans.append(0)
            stack.append(len(names) - 1)
        elif tok[0] == "End":
            end_site = True
        elif tok[0] == "}":
            if end_site:
                end_site = False
            else:
                stack.pop()
        elif tok[0] == "OFFSET" and not end_site:
            offsets[stack[-1]] = [float(v) for v in tok[1:4]]
        elif tok[0] == "CHANNELS":
            n = int(tok[1])
            chans[stack[-1]] = n
            rot = [c for c in tok[2:2 + n] if c in _CHAN]
            if order is None and len(rot) == 3:
                order = "".join(_CHAN[c] for c in rot)
        elif tok[0] == "MOTION":
            break
    # MOTION block: "Frames: N", "Frame Time: dt", then N rows of numbers -- parsed by the library's host helper (strtod on a few
    # threads: 7 200 rows x 228 numbers in ~8 ms, numpy.loadtxt 76 ms), numpy.loadtxt when it declines (ragged rows: loadtxt
    # raises the error the caller expects)
    off = mend
    probe = raw[off:off + 256]
    m1 = re.match(rb"\s*Frames:\s+(\d+)\s*?\n", probe)
    if m1 is None:
        raise ValueError(f"{filename}: the MOTION section does not start with 'Frames: <count>'")
    nframes = int(m1.group(1))
    m2 = re.match(rb"\s*Frame Time:\s+([\d\.eE\-\+]+)[^\n]*\n?", probe[m1.end():])
    if m2 is None:
        raise ValueError(f"{filename}: no 'Frame Time: <seconds>' line after 'Frames:'")
    frametime = float(m2.group(1))
    off += m1.end() + m2.end()                          # the rows start here; `raw` (a bytes object) ends in a NUL
    ncols = sum(chans)
    data = None
    if nframes > 0 and ncols > 0 and off < len(raw):
        out = np.empty((nframes, ncols), dtype=np.float64)
        base = C.cast(C.c_char_p(raw), C.c_void_p).value
        try:
            api().zeggs_parse_table_text(base + off, len(raw) - off, out.ctypes.data, nframes, int(ncols))
            data = out
        except RuntimeError:
            pass
    body = None
    if data is None:
        rows = [ln for ln in raw[off:].decode().splitlines() if ln.strip()][:nframes]
        data = np.loadtxt(rows, dtype=np.float64, ndmin=2) if rows else np.zeros((0, 0))     # C parser
    J = len(names)
    offsets = np.asarray(offsets, dtype=np.float32)
    positions = np.repeat(offsets[None], len(data), axis=0)
    rotations = np.zeros((len(data), J, 3), dtype=np.float32)
    col = 0
    for j in range(J):
        if chans[j] == 6:
            positions[:, j] = data[:, col:col + 3]
            rotations[:, j] = data[:, col + 3:col + 6]
        elif chans[j] == 3:
            rotations[:, j] = data[:, col:col + 3]
        else:
            raise ValueError(f"unsupported CHANNELS {chans[j]} on joint {names[j]}")
        col += chans[j]
    return dict(rotations=rotations, positions=positions, offsets=offsets, parents=np.asarray(parents, np.int32),
                names=names, order=order or "zyx", frametime=frametime)


def bvh_header(offsets, parents, names=None, order="zyx", nframes=0, frametime=1.0 / 60.0):
    """-> (text of the HIERARCHY block + the MOTION head, joint order of the motion rows) as reference bvh.save writes them
    (root with 6 channels, every other joint with 3, translations=False)."""
    offsets = np.asarray(offsets)
    parents = list(parents)
    names = names or [f"joint_{i}" for i in range(len(parents))]
    rot_ch = " ".join(_CHAN_INV[c] for c in order)
    children = {i: [j for j, p in enumerate(parents) if p == i] for i in range(len(parents))}
    seq, out = [], ["HIERARCHY"]

    def emit(i, depth):
        seq.append(i)
        ind = "\t" * depth
        out.append(f"{ind}{'ROOT' if depth == 0 else 'JOINT'} {names[i]}")
        out.append(ind + "{")
        out.append("%s\tOFFSET %f %f %f" % ((ind,) + tuple(offsets[i])))
        if depth == 0:
            out.append(f"{ind}\tCHANNELS 6 Xposition Yposition Zposition {rot_ch} ")
        else:
            out.append(f"{ind}\tCHANNELS 3 {rot_ch}")
        if children[i]:
            for c in children[i]:
                emit(c, depth + 1)
        else:
            out.extend([f"{ind}\tEnd Site", ind + "\t{", "%s\t\tOFFSET %f %f %f" % (ind, 0.0, 0.0, 0.0), ind + "\t}"])
        out.append(ind + "}")

    emit(0, 0)
    out += ["MOTION", "Frames: %i" % nframes, "Frame Time: %f" % frametime]
    return "\n".join(out) + "\n", seq


TEXT = "device"                   # default of the writers' `text=`: "device" (csrc/text.hip) or "host" (snprintf, hostio.hip)
TEXT_FALLBACKS = 0                # tables the device formatter handed back to the host one (a value outside its domain)
TEXT_UPLOAD_MIN_NUMBERS = 3648    # a HOST table goes through the device (upload + format + download) from this many numbers on
                                  # (16 rows of 228): measured 0.52 ms against the host's 0.76 ms there, 0.51 against 0.43 ms at 4
                                  # rows, and the device's cost stays under 0.8 ms up to 256 rows (profiles/bvh_text_device.json)


def _use_device_text(text, on_device, numbers):
    text = TEXT if text is None else text
    if text not in ("device", "host"):
        raise ValueError(f"text must be 'device' or 'host', not {text!r}")
    return text == "device" and numbers > 0 and (on_device or (numbers >= TEXT_UPLOAD_MIN_NUMBERS and torch.cuda.is_available()))


def bvh_save(filename, data, text=None):
    """Writes root with 6 channels and every other joint with 3 (reference bvh.save, translations=False).  `rotations` /
    `positions` may be host arrays or device tensors; text = "device" | "host" (None: anim.TEXT) chooses who formats the motion
    block: the device for device tensors and for host tables of TEXT_UPLOAD_MIN_NUMBERS numbers or more, else the host."""
    rots, poss = data["rotations"], data["positions"]
    head, seq = bvh_header(data["offsets"], data["parents"], data.get("names"), data.get("order", "zyx"), len(rots),
                           data.get("frametime", 1.0 / 60.0))
    on_device = torch.is_tensor(rots) and rots.is_cuda
    n = len(rots)
    if _use_device_text(text, on_device, n * (3 + 3 * len(seq))):
        # motion block: one row per frame = root position + the rotations in hierarchy order, built and formatted on the device
        dev = rots.device if on_device else torch.device("cuda")
        up = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dev, torch.float64)  # noqa: E731
        table = torch.cat([up(poss[:, 0]).reshape(n, 3),
                           up(rots)[:, torch.as_tensor(seq, device=dev)].reshape(n, 3 * len(seq))], dim=1).contiguous()
        with open(filename, "wb") as fh:
            fh.write(head.encode())
            fh.write(format_rows_device(table)[0])
        return
    if torch.is_tensor(rots):
        rots = rots.cpu().numpy()
    if torch.is_tensor(poss):
        poss = poss.cpu().numpy()
    rots, poss = np.asarray(rots), np.asarray(poss)
    table = np.concatenate([np.asarray(poss[:, 0], np.float64).reshape(len(rots), 3)] +
                           [np.asarray(rots[:, j], np.float64).reshape(len(rots), 3) for j in seq], axis=1)
    with open(filename, "w") as fh:
        fh.write(head)
    # the motion block is formatted by the library's host helper (same correctly-rounded "%f" as numpy.savetxt gives, ten
    # times faster: a 30-minute clip is 24.6 M numbers)
    table = np.ascontiguousarray(table, dtype=np.float64)
    try:
        api().zeggs_write_table_text(str(filename).encode(), 1, table.ctypes.data, table.shape[0], int(table.shape[1]))
    except RuntimeError as e:      # as np.savetxt / open() would: an OSError, which generate_gesture() reports and survives (generate.py:407)
        raise OSError(str(e)) from None


def format_rows(table, any_magnitude=False):
    """host float64 [rows, cols] (C-contiguous; e.g. a view of a pinned staging buffer) -> bytes of the BVH motion rows
    (zeggs_format_table_text: releases the GIL, so several host threads format row blocks side by side).  The buffer is sized
    for |values| < 1e15 (24 bytes per number); any_magnitude: for whatever a double can hold ("%f" of 1e308 has 309 digits)."""
    rows, cols = table.shape
    cap = rows * (cols * (330 if any_magnitude else 24) + 1) + 400
    buf = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    ptr = table.ctypes.data if isinstance(table, np.ndarray) else table.data_ptr()          # (host memory either way)
    api().zeggs_format_table_text(ptr, rows, int(cols), buf, cap, C.byref(n))
    return buf.raw[:n.value]


def table_text_device(table, cap=None):
    """device float64 [rows, cols] (contiguous) -> (text uint8 [cap] device, meta int64 [rows + 1] device), enqueued on the current
    stream (zeggs_table_text_device): text[:meta[rows - 1]] are the bytes format_rows gives, meta[:rows] the offset just past each
    row's line end, and the low 32 bits of meta[rows] the status word (bit 0: a value outside the digit routine's domain -- the text
    then holds a placeholder there and the caller formats the table on the host; bit 1: `cap` was too small)."""
    if not (table.is_cuda and table.dtype == torch.float64 and table.dim() == 2 and table.is_contiguous()):
        raise ValueError("table_text_device: a contiguous float64 [rows, cols] device tensor is expected")
    rows, cols = table.shape
    if rows == 0 or cols == 0:
        raise ValueError("table_text_device: empty table")
    L = api()
    cap = rows * (cols * 24 + 1) if cap is None else int(cap)
    text = torch.empty(cap, dtype=torch.uint8, device=table.device)
    meta = torch.empty(rows + 1, dtype=torch.int64, device=table.device)
    meta[rows:].zero_()
    ws = ops._ws(L.zeggs_table_text_workspace_bytes(rows, int(cols)), table.device)      # (stream-ordered: may go back to the allocator on return)
    L.zeggs_table_text_device(table, rows, int(cols), text, cap, meta, meta[rows:].view(torch.int32), ws, ws.numel(), ops._stream())
    return text, meta


def _host_pieces(table, bounds):
    """the out-of-domain rule, in one place: the table is downloaded and formatted by the host routine (snprintf: `nan`, `inf` and
    hundreds of digits included), and the event is counted"""
    global TEXT_FALLBACKS
    TEXT_FALLBACKS += 1
    host = np.ascontiguousarray(table.cpu().numpy())
    return [format_rows(host[a:b], any_magnitude=True) for a, b in zip(bounds[:-1], bounds[1:])]


def format_rows_device(table, cuts=None):
    """device float64 [rows, cols] -> the bytes of format_rows, formatted where the numbers are: the row ends come down first (8
    bytes per row), then exactly row_end[-1] bytes of text into pinned memory.  -> list of memoryview / bytes: the text cut in front
    of the rows `cuts` (ascending row indices; pieces of different clips share one table in the batch path), one piece without
    cuts.  A table with a value outside the device routine's domain (status word) is formatted by the host routine instead and
    counted in TEXT_FALLBACKS."""
    rows = table.shape[0]
    bounds = [0] + [int(c) for c in (cuts or [])] + [rows]
    if any(a > b for a, b in zip(bounds[:-1], bounds[1:])):
        raise ValueError("format_rows_device: cuts must be ascending row indices within the table")
    if rows == 0:
        return [b""] * (len(bounds) - 1)
    table = table.contiguous()
    text, meta = table_text_device(table)
    meta_h = meta.cpu().numpy()                         # (waits for the kernels)
    if int(meta_h[rows]) & 0xFFFFFFFF:
        return _host_pieces(table, bounds)
    total = int(meta_h[rows - 1])
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    host.copy_(text[:total], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    view = memoryview(host.numpy())
    ends = [0] + [int(x) for x in meta_h[:rows]]
    return [view[ends[a]:ends[b]] for a, b in zip(bounds[:-1], bounds[1:])]


# ----------------------------------------------------------------------------- device kernels (csrc/anim.hip)
def order_code(order):
    """'zyx' -> the packed channel order of ZeggsAnimDims / ZeggsBvhDims (axis of channel i in bits 2i..2i+1)"""
    if sorted(order) != ["x", "y", "z"]:
        raise ValueError(f"not a rotation channel order: {order!r}")
    return sum("xyz".index(c) << (2 * i) for i, c in enumerate(order))


ANIM_OUT = (("root_pos", 3, torch.float64), ("root_rot", 4, torch.float64), ("root_vel", 3, torch.float64),
            ("root_vrt", 3, torch.float64), ("lpos", -3, torch.float64), ("lrot", -4, torch.float64),
            ("lvel", -3, torch.float64), ("lvrt", -3, torch.float64), ("ltxy", -6, torch.float32),
            ("cpos", -3, torch.float64), ("crot", -4, torch.float64), ("cvel", -3, torch.float64),
            ("cvrt", -3, torch.float64), ("ctxy", -6, torch.float32), ("gaze_pos", 3, torch.float64),
            ("gaze_dir", 3, torch.float64))
assert tuple(n for n, _, _ in ANIM_OUT) == ANIM_OUT_FIELDS      # (the record itself: capi.AnimOut)


def preprocess_animation(anim, device=None):
    """BVH dict -> the 16 feature arrays of reference data_pipeline.preprocess_animation, same order:
    (root_pos, root_rot, root_vel, root_vrt, lpos, lrot, ltxy, lvel, lvrt, cpos, crot, ctxy, cvel, cvrt, gaze_pos,
    gaze_dir) as DEVICE tensors (float64; ltxy / ctxy float32)."""
    device = torch.device(device or "cuda")
    rot = torch.as_tensor(np.ascontiguousarray(anim["rotations"], dtype=np.float64), device=device)
    pos = torch.as_tensor(np.ascontiguousarray(anim["positions"], dtype=np.float64), device=device)
    return preprocess_animation_device(rot, pos, anim["parents"], anim["names"], anim["frametime"], anim["order"])


def preprocess_animation_device(rot, pos, parents, names, frametime, order):
    """preprocess_animation on channels that are on the device already: rot / pos float64 [N, J, 3] contiguous (what the
    dataset builder holds after trimming / stretching / centring a take)"""
    device = rot.device
    names = list(names)
    parents = torch.as_tensor(np.ascontiguousarray(parents, dtype=np.int32), device=device)
    N, J = rot.shape[0], rot.shape[1]
    d = AnimDims(N, J, names.index("Hips"), names.index("Spine2"), names.index("Head"), float(frametime),
                 order_code(order))      # any channel order (quat.from_euler takes any)
    L = api()
    ws = ops._ws(L.zeggs_anim_features_workspace_bytes(d), device)
    out, ptr = {}, AnimOut()
    for n, w, dt in ANIM_OUT:
        shape = (N, w) if w > 0 else ((N, J, 2, 3) if w == -6 else (N, J, -w))
        out[n] = torch.empty(shape, dtype=dt, device=device)
        setattr(ptr, n, out[n].data_ptr())
    L.zeggs_anim_features(d, parents, rot, pos, ptr, ws, ws.numel(), ops._stream())
    order = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "ltxy", "lvel", "lvrt", "cpos", "crot",
             "ctxy", "cvel", "cvrt", "gaze_pos", "gaze_dir")
    return tuple(out[k] for k in order)


def _to_euler_order(order):
    if order not in ("zyx", "xzy"):      # what quat.to_euler implements (ZEGGS/anim/quat.py:111-127); the reference raises the same
        raise NotImplementedError("Cannot convert to ordering %s" % order)
    return order_code(order)


def bvh_channels(root_pos, root_rot, lpos, ltxy, start_position=None, start_rotation=None, order="zyx"):
    """decoder output (device float32: [T,3], [T,4], [T,J,3], [T,J,2,3]) -> (positions, euler degrees) float64
    device tensors [T,J,3], channel order `order`, root folded into joint 0 (reference generate.py:389, utils.py:47-87)."""
    T, J = lpos.shape[0], lpos.shape[1]
    d = BvhDims(T, J, 0)
    d.order = _to_euler_order(order)
    if start_position is not None and start_rotation is not None:
        d.rebase = 1
        d.start_pos[:] = [float(v) for v in start_position]
        d.start_rot[:] = [float(v) for v in start_rotation]
    f = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    root_pos, root_rot, lpos, ltxy = f(root_pos), f(root_rot), f(lpos), f(ltxy)
    positions = torch.empty(T, J, 3, dtype=torch.float64, device=lpos.device)
    euler = torch.empty(T, J, 3, dtype=torch.float64, device=lpos.device)
    api().zeggs_pose_to_bvh(d, root_pos, root_rot, lpos, ltxy, positions, euler, ops._stream())
    return positions, euler


def plant_stage(parents, names, dt, device="cuda", max_frames=4096, **options):
    """a fresh one-row planting state (ops.LivePlant, reset) for plant_feet(..., stage=): what carries a clip's contact state from
    one piece of it to the next.  `options`: the keys of ops.PLANT_DEFAULTS (ops.plant_options checks them)."""
    conf = ops.plant_options(dict(options), parents, names)
    stage = ops.LivePlant(1, parents, max_frames, conf, dt, device)
    ops.live_plant_reset(stage, 0)
    return stage


def plant_feet(pose, rpos, rrot, parents, names, dt, stage=None, **options):
    """feet that stay planted (include/zeggs_hip_plant.h): the decoder's rows of a whole clip -- pose [T, 6 + 15J], rpos
    [T, 3], rrot [T, 4], float32 on the device -- through the contact lock and the leg IK, on the device -> (planted pose
    [T, 6 + 15J] float32: the ltxy of the chains' joints corrected, every other float the same bits; contacts [T, chains] uint8).
    `options`: chains="auto" | [(upper leg, lower leg, foot)] by name or index, speed=(v_on, v_off), height=(h_on, h_off), ground,
    slack, release, stretch (ops.PLANT_DEFAULTS: NOT tuned on captured motion).  A fresh one-row state a call; with `stage`
    (plant_stage) the state of the piece before is carried on and `options` are the stage's."""
    if stage is None:
        stage = plant_stage(parents, names, dt, pose.device, **options)
    elif options:
        raise ValueError("plant_feet: a stage carries its own options")
    f = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    pose, rpos, rrot = f(pose), f(rpos), f(rrot)
    T, PO = int(pose.shape[0]), stage.pose_floats
    if pose.dim() != 2 or pose.shape[1] != PO or tuple(rpos.shape) != (T, 3) or tuple(rrot.shape) != (T, 4):
        raise ValueError(f"plant_feet: pose [T, {PO}], rpos [T, 3], rrot [T, 4] for {stage.J} joints, not {tuple(pose.shape)}, {tuple(rpos.shape)}, "
                         f"{tuple(rrot.shape)}")
    out = torch.empty_like(pose)
    contacts = torch.zeros(T, stage.C, dtype=torch.uint8, device=pose.device)
    rec, M = (ops.PlantRow * 1)(), stage.d.max_frames
    for i in range(0, T, M):
        q = rec[0]
        q.pose, q.rpos, q.rrot = pose.data_ptr() + 4 * i * PO, rpos.data_ptr() + 12 * i, rrot.data_ptr() + 16 * i
        q.out, q.contacts = out.data_ptr() + 4 * i * PO, contacts.data_ptr() + i * stage.C
        q.pose_ld, q.rpos_ld, q.rrot_ld, q.out_ld, q.row, q.count = PO, 3, 4, PO, 0, min(M, T - i)
        ops.live_plant(stage, rec, 1)
    return out, contacts


def write_bvh(filename, root_pos, root_rot, lpos, ltxy, parents, names, order, dt, start_position=None,
              start_rotation=None, text=None):
    """reference utils.write_bvh, fed with the decoder's two-axis rotations (the quaternion / euler conversion of
    generate.py:389 happens on the device; text: see bvh_save)."""
    positions, euler = bvh_channels(root_pos, root_rot, lpos, ltxy, start_position, start_rotation, order)
    write_bvh_channels(filename, positions, euler, parents, names, order, dt, text=text)


def write_bvh_channels(filename, positions, euler, parents, names, order, dt, text=None):
    """the file half of write_bvh: device channel tables (bvh_channels) -> BVH text.  The channels stay on the device when the
    device formats them (text = "device", the default anim.TEXT); only frame 0's positions -- the OFFSETs -- come to the host."""
    if _use_device_text(text, positions.is_cuda, positions.shape[0] * positions.shape[1] * 3):
        bvh_save(filename, dict(order=order, offsets=positions[0].cpu().numpy(), names=names, frametime=dt, parents=parents,
                                positions=positions, rotations=euler), text="device")
        return
    positions = positions.cpu().numpy()
    bvh_save(filename, dict(order=order, offsets=positions[0], names=names, frametime=dt, parents=parents,
                            positions=positions, rotations=euler.cpu().numpy()), text="host")


# ----------------------------------------------------------------------------- left/right mirroring (csrc/mirror.hip)
# The pipeline's frame is fixed: forward +z, up +y, so left/right is x and the mirror plane is x = 0.  With M = diag(-1, 1, 1),
# M R_axis(t) M = R_axis(+t) about x and R_axis(-t) about y and z, factor by factor in any Euler order: a mirrored take is the
# original with paired joints exchanged, x positions negated and the y / z angles negated -- a permutation plus sign flips, for
# the BVH channels and, one level up, for every feature array.  One int32 per OUTPUT column says it: the source column in the
# low 31 bits, the sign flip in bit 31 (include/zeggs_hip_mirror.h).
_SEGMENT_SIGNS = {"vec": (-1, 1, 1),                  # a true vector: position, velocity, direction
                  "axial": (1, -1, -1),               # a pseudo-vector: angular velocity, helical
                  "quat": (1, 1, -1, -1),             # w, x, y, z
                  "txy": (1, -1, -1, -1, 1, 1)}       # the two-axis rotation rows: R ex mirrors as an axial, R ey as a vector
_FEATURE_KINDS = {"pos": "vec", "vel": "vec", "dir": "vec", "vrt": "axial", "rot": "quat", "txy": "txy"}     # by the name's ending


def _mirror_axis(axis):
    if axis != "x":
        raise NotImplementedError(f"mirror: the mirror plane is x = 0 (forward +z, up +y); axis={axis!r} is not implemented")


def segment_signs(kind, width=None):
    """signs of one block of a segment kind: vec | axial | quat | txy | euler:<order> | same (width floats, default 1)"""
    if kind in _SEGMENT_SIGNS:
        return _SEGMENT_SIGNS[kind]
    if kind.startswith("euler:"):
        order_code(kind[6:])                           # (raises for anything but a permutation of xyz)
        return tuple(1 if c == "x" else -1 for c in kind[6:])     # by the AXIS of a channel, not by its place
    if kind == "same":
        return (1,) * int(1 if width is None else width)
    raise ValueError(f"mirror: unknown segment kind {kind!r} (vec, axial, quat, txy, euler:<order>, same)")


def mirror_pairs(names, parents, left="Left", right="Right", axis="x"):
    """-> pair [J]: the joint a joint exchanges with under the left/right mirror, itself for a joint without a side.  A sided joint
    is one whose name holds `left` or `right`; its partner has the other word there.  ValueError (naming the joint) when a sided
    joint has no partner, or when the pairing is no automorphism of the tree: parents[pair[j]] != pair[parents[j]]."""
    _mirror_axis(axis)
    names = list(names)
    index = {n: i for i, n in enumerate(names)}
    pair = []
    for j, n in enumerate(names):
        other = n.replace(left, right, 1) if left in n else (n.replace(right, left, 1) if right in n else n)
        if other not in index:
            raise ValueError(f"mirror_pairs: joint {n!r} has no partner ({other!r} is not a joint)")
        pair.append(index[other])
    return _check_pairs(pair, names, parents)


def _check_pairs(pair, names, parents):
    J = len(parents)
    name = (lambda j: repr(names[j])) if names is not None else (lambda j: str(j))
    if len(pair) != J or any(not (0 <= int(p) < J) for p in pair):
        raise ValueError(f"mirror: a pairing of {len(pair)} entries for {J} joints (each 0 .. {J - 1})")
    pair = [int(p) for p in pair]
    for j in range(J):
        if pair[pair[j]] != j:
            raise ValueError(f"mirror: joint {name(j)} pairs with {name(pair[j])}, which pairs with {name(pair[pair[j]])}")
        pj, pp = int(parents[j]), int(parents[pair[j]])
        if pp != (pair[pj] if pj >= 0 else -1):
            raise ValueError(f"mirror: joint {name(j)} and its partner {name(pair[j])} hang under parents that are not partners "
                             "(the pairing is not an automorphism of the tree)")
    return pair


def resolve_pairs(pairs, names, parents, axis="x"):
    """what `pairs=` takes everywhere: "auto" (mirror_pairs by the names), an index list [J], or a dict of partners by name or
    index (one direction is enough; joints it does not mention pair with themselves) -> the checked index list"""
    _mirror_axis(axis)
    if isinstance(pairs, str):
        if pairs != "auto":
            raise ValueError(f"mirror: pairs={pairs!r} ('auto', a list or a dict)")
        return mirror_pairs(names, parents)
    if isinstance(pairs, dict):
        idx = lambda k: list(names).index(k) if isinstance(k, str) else int(k)  # noqa: E731
        out = list(range(len(parents)))
        for a, b in pairs.items():
            out[idx(a)], out[idx(b)] = idx(b), idx(a)
        pairs = out
    return _check_pairs(list(pairs), None if names is None else list(names), parents)


def named_layout(name, order="zyx"):
    """The row layouts the code base already states, as segment lists for mirror_table -- all of UN-normalised rows:
      "rotations" / "positions"   the BVH channel tables [F, J, 3] of bvh_load (euler degrees in channel order `order`; vectors)
      a feature of ANIM_OUT       "root_pos" .. "gaze_dir": one of the 16 arrays of preprocess_animation (kind by the name's
                                  ending, width and per-joint from ANIM_OUT); "Y_<feature>": the dataset key of the same array
      "decoder_in" / "example"    the decoder's input row of vectorize_input and the exemplar row of generate._example_features:
                                  the arrays of data_pipeline._IN_STATS one behind another, [9 + 15 J]
      "decoder_out"               the pose row of devectorize_output: data_pipeline._OUT_STATS, [6 + 15 J]"""
    if name == "rotations":
        return [("euler:" + order, "joint")]
    if name == "positions":
        return [("vec", "joint")]
    if name in ("decoder_in", "example", "decoder_out"):
        from . import data_pipeline
        keys = data_pipeline._OUT_STATS if name == "decoder_out" else data_pipeline._IN_STATS
        return [seg for k in keys for seg in named_layout(k)]
    feature = name[2:] if name.startswith("Y_") else name
    widths = {n: w for n, w, _ in ANIM_OUT}
    if feature not in widths:
        raise ValueError(f"mirror: no row layout called {name!r}")
    kind = _FEATURE_KINDS[feature[-3:]]
    assert len(segment_signs(kind)) == abs(widths[feature]), feature
    return [(kind, "joint" if widths[feature] < 0 else "single")]


def mirror_table(layout, pairs, axis="x", order="zyx"):
    """-> int32 [cols]: the signed column table of a row layout (include/zeggs_hip_mirror.h).  `layout`: a name of named_layout
    (`order`: the channel order of "rotations") or a sequence of segments (kind, scope[, width]) -- kind as in segment_signs,
    scope "joint" (one block per joint in joint order, block j read from block pairs[j]) or "single" (one block), width for
    "same".  `pairs`: the checked index list (mirror_pairs / resolve_pairs)."""
    _mirror_axis(axis)
    segments = named_layout(layout, order) if isinstance(layout, str) else list(layout)
    pairs = [int(p) for p in pairs]
    if sorted(pairs) != list(range(len(pairs))):
        raise ValueError("mirror_table: pairs is not a permutation of the joints")
    table, off = [], 0
    for seg in segments:
        kind, scope = seg[0], seg[1]
        signs = segment_signs(kind, seg[2] if len(seg) > 2 else None)
        if scope not in ("joint", "single"):
            raise ValueError(f"mirror_table: scope {scope!r} of segment {seg!r} ('joint' or 'single')")
        blocks = pairs if scope == "joint" else [0]
        w = len(signs)
        for src in blocks:
            table += [(off + src * w + k) | (0x80000000 if s < 0 else 0) for k, s in enumerate(signs)]
        off += w * len(blocks)
    return np.asarray(table, dtype=np.uint32).view(np.int32)


def check_mirror_table(table):
    """ValueError unless every column is the source of exactly one column (the check the library makes before it builds a plan)"""
    table = np.ascontiguousarray(table, dtype=np.int32)
    try:
        api().zeggs_mirror_table_check(table.ctypes.data, int(table.size))
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    return table


def mirror_rows_host(x, table):
    """the kernel's statement in NumPy: out[..., c] = x[..., source(c)] with the sign bit flipped where bit 31 of table[c] is set
    (float32 or float64; an exclusive-or on the integer view, so -0.0, infinities and NaN payloads keep their other bits)"""
    x = np.ascontiguousarray(x)
    bits = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    t = np.asarray(table, dtype=np.int32).view(np.uint32)
    flat = x.reshape(-1, t.size).view(bits)
    flip = ((t >> 31).astype(bits) << bits(8 * x.dtype.itemsize - 1))
    return (flat[:, t & 0x7FFFFFFF] ^ flip[None]).view(x.dtype).reshape(x.shape)


class _MirrorPlan:
    """a plan of the library (the table on the device); freed with the object"""

    def __init__(self, table):
        self.table = np.ascontiguousarray(table, dtype=np.int32)
        self.handle = C.c_void_p()
        api().zeggs_mirror_plan_create(self.table.ctypes.data, int(self.table.size), C.addressof(self.handle))

    def __del__(self):
        try:
            if self.handle:
                api().zeggs_mirror_plan_free(self.handle)
        except Exception:          # (interpreter shutdown)
            pass


_MIRROR_PLANS = {}            # (device, table bytes) -> plan, the most recently used last; at most _MIRROR_PLANS_MAX of them
_MIRROR_PLANS_MAX = 64        # (a rig has some twenty layouts; an evicted plan is freed when its last user lets go of it)
_MIRROR_TABLES = {}           # (layout name, pairs, order) -> table: building one is a Python loop over its columns


def _mirror_plan(table, device):
    key = (device.index if device.index is not None else torch.cuda.current_device(), table.tobytes())
    plan = _MIRROR_PLANS.pop(key, None)
    if plan is None:
        with torch.cuda.device(key[0]):
            plan = _MirrorPlan(table)
        while len(_MIRROR_PLANS) >= _MIRROR_PLANS_MAX:
            del _MIRROR_PLANS[next(iter(_MIRROR_PLANS))]
    _MIRROR_PLANS[key] = plan
    return plan


def _mirror_table_of(layout, pairs, axis, order):
    """mirror_table, kept per (name, pairs, order) for the named layouts"""
    if not isinstance(layout, str):
        return mirror_table(layout, pairs, axis, order)
    key = (layout, tuple(int(p) for p in pairs), order)
    table = _MIRROR_TABLES.get(key)
    if table is None:
        if len(_MIRROR_TABLES) >= _MIRROR_PLANS_MAX:
            _MIRROR_TABLES.clear()
        table = _MIRROR_TABLES[key] = mirror_table(layout, pairs, axis, order)
    return table


def mirror_rows(x, layout, pairs=None, axis="x", order="zyx"):
    """x: device tensor (float32 or float64) whose trailing dimensions flatten to the rows of `layout` -> its left/right mirror, a new
    tensor of the same shape: ONE launch of the signed column gather.  `layout`: as in mirror_table, or a ready int32 table
    (`pairs` is then not needed).  The table of a named layout is built on its first use and kept per (name, pairs, order); the
    plan -- the table on the device -- is made on first use of a table and kept, the 64 most recently used per process."""
    _mirror_axis(axis)
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise RuntimeError("mirror_rows: a float32 or float64 tensor on the GPU is needed (the HIP engine has no CPU path)")
    table = np.ascontiguousarray(layout, np.int32) if isinstance(layout, np.ndarray) else _mirror_table_of(layout, pairs, axis, order)
    cols = int(table.size)
    trailing = list(np.cumprod([1] + list(x.shape[::-1])))          # a row is some number of whole trailing dimensions
    if cols not in trailing:
        raise ValueError(f"mirror_rows: a tensor of shape {tuple(x.shape)} does not hold rows of {cols} columns")
    x = x.contiguous()
    out = torch.empty_like(x)
    plan = _mirror_plan(table, x.device)
    with torch.cuda.device(x.device):
        api().zeggs_mirror_rows(plan.handle, x, out, x.numel() // cols, x.element_size(), ops._stream())
    return out


def rig_asymmetry(offsets, pairs):
    """the largest distance between a joint's offset and the reflection of its partner's offset, relative to the bone's length
    (0 for a rig that is its own mirror image; a bone of length 0 counts with a length of 1)"""
    off = np.asarray(offsets, dtype=np.float64)
    if off.size == 0:
        return 0.0
    refl = off[np.asarray(pairs)] * np.array([-1.0, 1.0, 1.0])
    length = np.linalg.norm(off, axis=-1)
    return float(np.max(np.linalg.norm(off - refl, axis=-1) / np.where(length > 0.0, length, 1.0)))


def mirror_take(take, pairs="auto", symmetry_tol=None, axis="x"):
    """take: the dict of bvh_load -- `rotations` / `positions` [F, J, 3] as host arrays or as device tensors (float32 / float64)
    -> the left/right mirrored take: paired joints exchanged, x positions and the angles about y and z negated (exactly: only
    sign bits change), `offsets[pair]` with x negated, the same names, parents, order and frametime; device tensors go through
    the kernel (one launch each) and stay on the device.  `take["asymmetry"]` reports rig_asymmetry of the ORIGINAL's offsets;
    an asymmetric rig is mirrored all the same (its bones then change length with the side) unless `symmetry_tol` is given:
    ValueError above it."""
    _mirror_axis(axis)
    pair = resolve_pairs(pairs, take.get("names"), take["parents"])
    offsets = take["offsets"].cpu().numpy() if torch.is_tensor(take["offsets"]) else np.asarray(take["offsets"])
    asym = rig_asymmetry(offsets, pair)
    if symmetry_tol is not None and not asym <= symmetry_tol:
        raise ValueError(f"mirror_take: the rig's asymmetry is {asym:.6g}, above symmetry_tol = {symmetry_tol}")
    order = take.get("order", "zyx")
    tables = {"rotations": mirror_table("rotations", pair, order=order), "positions": mirror_table("positions", pair)}
    out = dict(take)
    for k, t in tables.items():
        a = take[k]
        if torch.is_tensor(a) and a.is_cuda:
            out[k] = mirror_rows(a, t)
        else:
            out[k] = mirror_rows_host(a.numpy() if torch.is_tensor(a) else np.asarray(a), t)
    out["offsets"] = mirror_rows_host(np.ascontiguousarray(offsets).reshape(1, -1), tables["positions"]).reshape(offsets.shape)
    out["asymmetry"] = asym
    return out
