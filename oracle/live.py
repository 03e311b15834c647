"""The incremental speech encoder of live serving (csrc/live.hip: live_speech_k) restated on the host, in any dtype.

Same scheme, no shared code: per-row rings of D frames with frame f in slot f % D, layer 0 computed once per frame when its
feature row arrives, an output frame f read from the taps f - half .. f + half clamped to [0, top] (top = the row's last frame
once it is known, else the newest frame in the ring), driven by the same per-row records (n_ring, k0, last, n_new, n_out,
feat_off).  tests/test_live_encoder_oracle_cpu.py holds it to oracle.nets.speech_encoder on the whole row (1e-12 in float64) and
uses its `bug` switches as negative controls for the bound of tests/test_gpu_live_dims.py.

Also here: the argument checks of zeggs_speech_encoder_live / live_dims_ok restated (check_dims, check_row) -- what the C side
refuses ahead of a launch, as the message fragment a caller can match on."""
import torch
import torch.nn.functional as F

LTHR, MAX_ROWS, LDS_LIMIT = 512, 64, 64 * 1024
BUGS = ("top_off_by_one", "slot_plus_one", "taps_reversed", "lap_late", "zero_padding", "pack_h_o_swapped")


def lds_bytes(Fd, H, O, KW):
    """live_lds: act [FRP + KW - 1][H] | xs [FA][F] rounded up to 4 floats | h1s [FRP][O]"""
    FRP, FA = LTHR // O, LTHR // H
    return 4 * ((FRP + KW - 1) * H + (FA * Fd + 3) // 4 * 4 + FRP * O)


def check_dims(R, Fd, H, O, KW, D, feat_ld, out_ld):
    """live_dims_ok -> None or the fragment of the message the first failing check gives"""
    if not 1 <= R <= MAX_ROWS:
        return f"{R} rows"
    if KW % 2 != 1 or KW < 1:
        return "even kernel width"
    if not (Fd >= 1 and H >= 4 and O >= 4 and H % 4 == 0 and O % 4 == 0 and LTHR % H == 0 and LTHR % O == 0):
        return "must be multiples of 4 that divide"
    if not (D >= KW and feat_ld >= 1 and out_ld >= 1):
        return "frames under a kernel of"
    if lds_bytes(Fd, H, O, KW) > LDS_LIMIT:
        return "bytes of LDS"
    return None


def check_row(rec, KW, D, feat_ld, out_ld):
    """the per-row loop of zeggs_speech_encoder_live; rec = (n_ring, k0, last, n_new, n_out, feat_off) -> None or the fragment"""
    n_ring, k0, last, n_new, n_out, feat_off = rec
    half = (KW - 1) // 2
    if n_new < 0 or n_out < 0 or n_ring < 0 or feat_off < 0:
        return "negative count"
    if n_new > D or feat_off + n_new > feat_ld:
        return "new frames at"
    if n_out > out_ld:
        return "output rows"
    total = n_ring + n_new
    if last >= 0 and total != last + 1:
        return "ended at frame"
    if n_out > 0:
        if k0 < 0 or total < 1:
            return "nothing to read"
        lo, hi = max(k0 - half, 0), k0 + n_out - 1 + half
        if last >= 0:
            if k0 + n_out - 1 > last:
                return "past the last one"
            hi, lo = min(hi, last), min(lo, last)
        if hi >= total:
            return "needs frame"
        if lo < total - D:
            return "left the ring"
    return None


def pack_w1(w1):
    """live_pack_k: [O, H, KW] -> flat [KW][H/4][O][4]"""
    O, H, KW = w1.shape
    return w1.permute(2, 1, 0).reshape(KW, H // 4, 4, O).permute(0, 1, 3, 2).reshape(-1)


def unpack_w1(p, O, H, KW, swapped=False):
    """the element the kernel's conv loop reads for (tap j, channel 4 c4 + e, output o): flat index ((j H/4 + c4) O + o) 4 + e
    -> [O, H, KW].  swapped: H and O exchanged in that index, ((j O/4 + c4) H + o) 4 + e, taken modulo one tap's H O floats"""
    j = torch.arange(KW).view(KW, 1, 1, 1)
    c4 = torch.arange(H // 4).view(1, H // 4, 1, 1)
    e = torch.arange(4).view(1, 1, 4, 1)
    o = torch.arange(O).view(1, 1, 1, O)
    if swapped:
        idx = j * H * O + ((c4 * H + o) * 4 + e) % (H * O)
    else:
        idx = ((j * (H // 4) + c4) * O + o) * 4 + e
    return p[idx].reshape(KW, H, O).permute(2, 1, 0).contiguous()


def encoder_incremental(w, mean, std, blocks, calls, R, D, dtype=torch.float64, bug=None):
    """w: dict layer0/1/2.weight/.bias (layer0.weight [H, F] or [H, F, 1]); mean, std [F]; blocks(c) -> the float32 feature block
    [R, feat_ld, F] of call c, un-normalised; calls: per call R records (n_ring, k0, last, n_new, n_out, feat_off).
    -> per row the produced frames in order, [n, O] in `dtype`."""
    assert bug is None or bug in BUGS, bug
    t = lambda a: a.detach().cpu().to(dtype)  # noqa: E731
    w0, b0, w1, b1, w2, b2 = (t(w[f"layer{i}.{k}"]) for i in range(3) for k in ("weight", "bias"))
    w0 = w0.reshape(w0.shape[0], -1)
    O, H, KW = w1.shape
    half = (KW - 1) // 2
    w1 = unpack_w1(pack_w1(w1), O, H, KW, swapped=bug == "pack_h_o_swapped")
    if bug == "taps_reversed":
        w1 = w1.flip(2)
    mean, std = t(mean), t(std)
    ring = torch.zeros(R, D, H, dtype=dtype)
    got = [[] for _ in range(R)]
    for c, recs in enumerate(calls):
        blk = None
        for r, (n_ring, k0, last, n_new, n_out, feat_off) in enumerate(recs):
            if n_new == 0 and n_out == 0:
                continue
            stale = ring[r].clone()
            if n_new:
                blk = blocks(c) if blk is None else blk
                x = (t(blk[r, feat_off:feat_off + n_new]) - mean) / std
                slots = (n_ring + torch.arange(n_new)) % D
                ring[r, slots] = F.elu(x @ w0.T + b0)
            if n_out == 0:
                continue
            top = last if last >= 0 else n_ring + n_new - 1
            if bug == "top_off_by_one":
                top = max(top - 1, 0)
            q = (k0 + torch.arange(n_out)).view(-1, 1) + torch.arange(KW).view(1, -1) - half
            inside = (q >= 0) & (q <= top)
            q = q.clamp(0, top)
            src = stale if bug == "lap_late" else ring[r]
            a = src[(q + 1) % D if bug == "slot_plus_one" else q % D]           # [n_out, KW, H]
            if bug == "zero_padding":
                a = a * inside.unsqueeze(-1).to(dtype)
            h1 = F.elu(torch.einsum("nkh,ohk->no", a, w1) + b1)
            got[r].append(F.elu(h1 @ w2.T + b2))
    O_ = w2.shape[0]
    return [torch.cat(g) if g else torch.zeros(0, O_, dtype=dtype) for g in got]
