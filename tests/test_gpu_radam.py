"""RAdam on the device past step 5 -- radam_k through ops.radam_step, zeggs.optimizers.RAdam (per-tensor, flat with early()
slices, resume, rewind) and TrainEngine's optimizer step -- against the float64 oracle (oracle/radam.py), p, exp_avg AND
exp_avg_sq, in float32 roundings per element and step.

The bound is helpers.RADAM_BOUND = 4 x the distance of the reference's own float32 run from the same oracle (p 26, m 16.8, v 28
roundings; measured and justified in tests/test_radam_oracle_cpu.py, which also proves that eight one-line mistakes are at least
10 x outside it and that complements formed in float32 -- what the kernel did before -- are 223 roundings off in v).
The module prints its worst roundings per array when it ends (run with -s); DESIGN.md section 5 records them."""
import copy

import numpy as np
import pytest
import torch

import helpers
from oracle import radam as oradam
from zeggs import engine, ops, optimizers, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
WORST = dict(p=0.0, m=0.0, v=0.0)
WORST_TEST = dict(p=0.0, m=0.0, v=0.0)
# (weight_decay, degenerated_to_sgd): plain; decay in both forms; step_scale = 0 at the steps before the rectified ones
FORMS = {"plain": (0.0, True), "decay": (0.05, True), "no-sgd": (0.0, False)}


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _note(worst, tag):
    for k in "pmv":
        WORST[k], WORST_TEST[k] = max(WORST[k], worst[k]), max(WORST_TEST[k], worst[k])
    for k in "pmv":
        assert worst[k] <= helpers.RADAM_BOUND[k], \
            f"{tag}: {k} is {worst[k]:.1f} float32 roundings from the float64 oracle (bound {helpers.RADAM_BOUND[k]:.1f})"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ntest_gpu_radam.py: worst float32 roundings from the float64 oracle " +
          ", ".join(f"{k} {WORST[k]:.2f} (bound {helpers.RADAM_BOUND[k]:.1f})" for k in "pmv"))


@pytest.fixture(autouse=True)
def _report_test(request):
    WORST_TEST.update(p=0.0, m=0.0, v=0.0)
    yield
    if any(WORST_TEST.values()):
        print(f"\n{request.node.name}: worst roundings " + ", ".join(f"{k} {WORST_TEST[k]:.2f}" for k in "pmv"))


def _kernel_args(step, lr, weight_decay, degenerated_to_sgd, betas=(0.9, 0.999)):
    """-> (step_scale, rectified, decay) as a caller of the C entry point passes them"""
    rect, scale = oradam.radam_scalars(step, lr, betas[0], betas[1], degenerated_to_sgd)
    if scale is None:
        return 0.0, False, 0.0
    return scale, rect, weight_decay * lr


def _kernel_run(p, gr, m, v, steps, lr, form, **kw):
    """ops.radam_step over `steps` (1-based) on device tensors p, m, v in place, grads gr[i]; -> dict p, m, v [len(steps), n]"""
    wd, degen = FORMS[form]
    out = {k: [] for k in "pmv"}
    for i, step in enumerate(steps):
        scale, rect, decay = _kernel_args(step, lr, wd, degen)
        ops.radam_step(p, gr[i], m, v, 0.9, 0.999, EPS, scale, rect, decay=decay, **kw)
        for k, t in zip("pmv", (p, m, v)):
            out[k].append(t.clone())
    return {k: torch.stack(a).cpu().numpy() for k, a in out.items()}


# ----------------------------------------------------------------------------- the kernel
SIZES = (1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1025)     # n4 = 0 (tail only), tails of 0-3, a second workgroup (n4 = 256 at 1024)


@pytest.mark.parametrize("form", list(FORMS))
def test_kernel_sizes_steps_1_to_8(form):
    """n from 1 (no 16-byte body at all) over every tail length to two workgroups, steps 1...8: the unrectified form at steps
    1-5 (with step_scale = 0 under degenerated_to_sgd=False), the rectified one from step 6, with and without decay."""
    wd, degen = FORMS[form]
    steps = range(1, 9)
    for n in SIZES:
        p0, gr, never, _ = oradam.recipe(n, len(steps), seed=100 + n)
        ref = helpers.radam_oracle_run(p0, gr, steps, 1e-2, EPS, weight_decay=wd, degenerated_to_sgd=degen)
        p = g(p0)
        got = _kernel_run(p, [g(a) for a in gr], torch.zeros_like(p), torch.zeros_like(p), steps, 1e-2, form)
        _note(helpers.radam_worst(got, ref), f"{form} n={n}")
        assert not got["m"][:, never].any() and not got["v"][:, never].any()
        if form == "no-sgd":
            assert np.array_equal(got["p"][4], p0) and not np.array_equal(got["p"][5], p0)


def test_kernel_grid_stride_loop():
    """n = 8 388 608 + 3 * 1024 + 7: the grid is capped at 8192 workgroups of 256 x 4 elements, so the last 3 * 1024 + 4 elements
    are a second trip of the loop and 3 a tail behind it; steps 5 and 6 (both forms) with decay.  The oracle runs in float64 on the
    device.  The inputs are the recipe's at n = 1 000 003 repeated: a period that does not divide the loop's stride."""
    n, period, steps, lr = 8388608 + 3 * 1024 + 7, 1000003, (5, 6), 1e-2
    p0, gr, _, _ = oradam.recipe(period, len(steps), seed=7)
    p0, gr = g(np.resize(p0, n)), [g(np.resize(a, n)) for a in gr]       # (each gradient 16-byte aligned: an allocation of its own)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    p64, m64, v64 = p0.double(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    path, mabs = p64.abs(), torch.zeros_like(p64)
    for i, step in enumerate(steps):
        scale, rect, decay = _kernel_args(step, lr, 0.05, True)
        ops.radam_step(p, gr[i], m, v, 0.9, 0.999, EPS, scale, rect, decay=decay)
        before = p64.clone()
        oradam.radam_step(p64, gr[i].double(), m64, v64, step, lr, EPS, weight_decay=0.05)
        path, mabs = path + (p64 - before).abs(), 0.9 * mabs + (1 - 0.9) * gr[i].double().abs()
        _note({k: helpers.radam_roundings_torch(a, r, s) for k, a, r, s in zip("pmv", (p, m, v), (p64, m64, v64), (path, mabs, v64))},
              f"n={n} step {step}")
    assert float((p != p0)[8388608:].float().mean()) > 0.9             # the second trip and the tail were stepped


@pytest.mark.parametrize("lo,length", [(lo, ln) for lo in (4, 260) for ln in (5, 1026)])
def test_kernel_slice_leaves_its_neighbours_alone(lo, length):
    """A slice [lo, hi) of larger buffers (what RAdam.early and the remainder pass), steps 5-7: inside, the oracle's values; outside,
    every element of all four buffers -- live values, not zeros -- bit-identical afterwards."""
    hi, N, steps = lo + length, 1400, (5, 6, 7)
    p0, gr, _, _ = oradam.recipe(length, len(steps), seed=lo + length)
    marks = dict(p=7.25, g=-3.5, m=0.375, v=13.0)
    buf = {k: torch.full((N,), val, device=DEV) for k, val in marks.items()}
    buf["p"][lo:hi] = g(p0)
    buf["m"][lo:hi] = 0
    buf["v"][lo:hi] = 0
    wd, degen = FORMS["decay"]
    ref = helpers.radam_oracle_run(p0, gr, steps, 1e-2, EPS, weight_decay=wd, degenerated_to_sgd=degen)
    out = {k: [] for k in "pmv"}
    for i, step in enumerate(steps):
        buf["g"][lo:hi] = g(gr[i])
        scale, rect, decay = _kernel_args(step, 1e-2, wd, degen)
        ops.radam_step(buf["p"][lo:hi], buf["g"][lo:hi], buf["m"][lo:hi], buf["v"][lo:hi], 0.9, 0.999, EPS, scale, rect, decay=decay)
        for k in "pmv":
            out[k].append(buf[k][lo:hi].clone())
    _note(helpers.radam_worst({k: torch.stack(a).cpu().numpy() for k, a in out.items()}, ref), f"slice [{lo}, {hi})")
    for k, val in marks.items():
        outside = torch.cat([buf[k][:lo], buf[k][hi:]])
        assert torch.equal(outside.view(torch.int32), torch.full_like(outside, val).view(torch.int32)), k
    assert torch.equal(buf["g"][lo:hi], g(gr[-1]))


def test_kernel_guarded_entry():
    """status[0] != 0 (written by the host) or gflag != 0: p, m, v bit-identical, status[1] + 1 only where `count` is set; both
    zero: bit-equal to the unguarded call."""
    n, step = 1025, 6
    p0, gr, _, _ = oradam.recipe(n, 2, seed=3)
    scale, rect, decay = _kernel_args(step, 1e-2, 0.05, True)

    def state():
        p, m, v = g(p0), g(np.abs(gr[1]) * 0.1), g(gr[1] * gr[1] * 0.01)
        return p, g(gr[0]), m, v

    def call(s, **kw):
        ops.radam_step(s[0], s[1], s[2], s[3], 0.9, 0.999, EPS, scale, rect, decay=decay, **kw)

    plain = state()
    call(plain)
    assert not torch.equal(plain[0], g(p0))
    for flagged in ("status", "gflag"):
        status = ops.new_status(DEV)
        gflag = torch.zeros(4, device=DEV)
        if flagged == "status":
            status[0] = 1
        else:
            gflag[0] = 1.0
        s, keep = state(), state()
        for count, expect in ((True, 1), (False, 1), (True, 2)):
            call(s, status=status, gflag=gflag[:1], count=count)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(s, keep)), (flagged, count)
            assert status.cpu().tolist() == [int(flagged == "status"), expect, 0, 0]
    for gflag in (None, torch.zeros(4, device=DEV)[:1]):
        status, s = ops.new_status(DEV), state()
        call(s, status=status, gflag=gflag, count=True)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(s, plain))
        assert status.cpu().tolist() == [0, 0, 0, 0]


# ----------------------------------------------------------------------------- the optimizer class
def _lr_decay(opt, step):
    gd = helpers.radam_fixture()[0]
    if step == int(gd["decay_before_step"]):
        for grp in opt.param_groups:
            grp["lr"] *= float(gd["lr_decay"])


def _oracle(conf, steps=12):
    return [helpers.radam_oracle_run(d["p0"], d["g"], range(1, steps + 1), d["lr"], EPS, d["betas"], d["weight_decay"],
                                     d["degenerated_to_sgd"]) for d in conf]


def _new_opt(conf, params):
    ngroups = 1 + max(d["group"] for d in conf)
    groups = []
    for k in range(ngroups):
        first = next(d for d in conf if d["group"] == k)
        groups.append(dict(params=[q for q, d in zip(params, conf) if d["group"] == k], lr=first["lr"], betas=first["betas"]))
    return optimizers.RAdam(groups, eps=EPS, weight_decay=conf[0]["weight_decay"], degenerated_to_sgd=conf[0]["degenerated_to_sgd"])


def _against_fixture(conf, refs, t, s, got, tag):
    """one tensor after step s + 1 against the float64 oracle at the bound, and against the reference's own float32 values at the
    bound + the reference's own distance (helpers.RADAM_REF_ROUNDINGS)"""
    d, ref = conf[t], refs[t]
    got = {k: a.detach().cpu().numpy().reshape(1, -1) for k, a in got.items()}
    _note({k: helpers.radam_roundings(got[k], ref[k][s:s + 1], ref["s" + k][s:s + 1]) for k in "pmv"}, f"{tag} tensor {t} step {s + 1}")
    for k in "pmv":
        r = helpers.radam_roundings(got[k], d[k][s:s + 1].astype(np.float64), ref["s" + k][s:s + 1])
        assert r <= helpers.RADAM_BOUND[k] + helpers.RADAM_REF_ROUNDINGS[k], (tag, t, s + 1, k, r)


@pytest.mark.parametrize("c", range(4))
def test_class_per_tensor_vs_reference(c):
    """zeggs.optimizers.RAdam, one launch per tensor, all four configurations of radam_steps.npz (the fourth: two parameter groups
    with their own lr and betas), lr decayed on param_groups before step 9: p, exp_avg, exp_avg_sq of every tensor at every step."""
    gd, configs = helpers.radam_fixture()
    conf, refs = configs[c], _oracle(configs[c])
    params = [torch.nn.Parameter(g(d["p0"].reshape(d["shape"]))) for d in conf]
    opt = _new_opt(conf, params)
    for s in range(int(gd["steps"])):
        _lr_decay(opt, s + 1)
        for q, d in zip(params, conf):
            q.grad = g(d["g"][s].reshape(d["shape"]))
        opt.step()
        for t, q in enumerate(params):
            st = opt.state[q]
            assert st["step"] == s + 1 and st["exp_avg"].shape == q.shape
            _against_fixture(conf, refs, t, s, dict(p=q, m=st["exp_avg"], v=st["exp_avg_sq"]), f"per-tensor config {c}")


class _Flat:
    """the three tensors of a configuration as views of one flat buffer (zeggs.engine.flatten_parameters' layout), a flat
    optimizer over them and its step split by early() at `slices`"""

    def __init__(self, conf, slices, guard, p_init=None):
        self.conf, self.slices = conf, slices
        sizes = [d["p0"].size for d in conf]
        self.offs = np.concatenate([[0], np.cumsum(sizes)])
        self.fp = g(np.concatenate([d["p0"] for d in conf])) if p_init is None else p_init.clone()
        self.fg = torch.zeros_like(self.fp)
        self.params = []
        for t, d in enumerate(conf):
            q = torch.nn.Parameter(torch.empty(0, device=DEV))
            q.data = self.fp[self.offs[t]:self.offs[t + 1]].view(d["shape"])
            q.grad = self.fg[self.offs[t]:self.offs[t + 1]].view(d["shape"])
            self.params.append(q)
        self.opt = _new_opt(conf, self.params)
        self.status = ops.new_status(DEV) if guard else None

    def attach(self, keep_state=False):
        self.opt.attach_flat(self.fp, self.fg, keep_state=keep_state)
        if self.status is not None:
            self.opt.attach_guard(self.status)
        return self

    def step(self, s):
        """step s + 1 of the fixture"""
        _lr_decay(self.opt, s + 1)
        self.fg.copy_(g(np.concatenate([d["g"][s] for d in self.conf])))
        for lo, hi in self.slices:
            self.opt.early(lo, hi)
        self.opt.step()
        return self.snapshot()

    def snapshot(self):
        return tuple(t.clone() for t in (self.fp, self.opt._flat[2], self.opt._flat[3]))


SLICES = {"one-slice": ((4, 268),), "two-slices": ((8, 12), (300, 636))}


@pytest.mark.parametrize("slices", list(SLICES))
@pytest.mark.parametrize("c", range(3))
def test_class_flat_with_early_slices_vs_reference(c, slices):
    """The flat path as the engine drives it: part of the coming step applied by early(), the remainder by step() -- through the
    guarded entry point in the two-slices runs -- for the three single-group configurations; every tensor's p, exp_avg and
    exp_avg_sq (the state views a checkpoint saves) at every step."""
    gd, configs = helpers.radam_fixture()
    conf, refs = configs[c], _oracle(configs[c])
    f = _Flat(conf, SLICES[slices], guard=slices == "two-slices").attach()
    for s in range(int(gd["steps"])):
        f.step(s)
        for t, q in enumerate(f.params):
            st = f.opt.state[q]
            assert st["step"] == s + 1 and st["exp_avg"].data_ptr() == f.opt._flat[2][f.offs[t]:].data_ptr()
            _against_fixture(conf, refs, t, s, dict(p=q, m=st["exp_avg"], v=st["exp_avg_sq"]), f"flat {slices} config {c}")
    assert f.opt.early_pieces == len(SLICES[slices]) * int(gd["steps"]) and f.opt._early == []
    if f.status is not None:
        assert f.status.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("k", [4, 7])
def test_class_resume_is_bit_equal(k):
    """k steps, state_dict() into a fresh optimizer over fresh buffers (load_state_dict, attach_flat(keep_state=True)), the
    remaining steps: every later step bit-equal to the uninterrupted run -- k = 4 resumes inside the unrectified steps, k = 7
    behind the boundary."""
    gd, configs = helpers.radam_fixture()
    conf, steps = configs[1], int(gd["steps"])
    whole = _Flat(conf, SLICES["one-slice"], guard=True).attach()
    want = [whole.step(s) for s in range(steps)]
    first = _Flat(conf, SLICES["one-slice"], guard=True).attach()
    for s in range(k):
        first.step(s)
    sd = copy.deepcopy(first.opt.state_dict())
    second = _Flat(conf, SLICES["one-slice"], guard=True, p_init=first.fp)
    second.opt.load_state_dict(sd)
    moments = [(second.opt.state[q]["exp_avg"].clone(), second.opt.state[q]["exp_avg_sq"].clone()) for q in second.params]
    second.attach(keep_state=True)
    assert second.opt._step == k
    for q, (m, v) in zip(second.params, moments):        # the checkpoint's moments, now views of the new flat buffers
        assert torch.equal(second.opt.state[q]["exp_avg"], m) and torch.equal(second.opt.state[q]["exp_avg_sq"], v)
    assert all(torch.equal(a, b) for a, b in zip(second.snapshot(), want[k - 1]))
    for s in range(k, steps):
        got = second.step(s)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want[s])), f"step {s + 1} after resuming at {k}"


def test_class_rewind_after_skipped_steps_is_bit_equal():
    """Steps 6 and 7 skipped ON THE DEVICE through the guard (both pieces of each), counted once each; then the status words
    zeroed, rewind(2), and the two steps run again: bit-equal to the run that never skipped, to the last step."""
    gd, configs = helpers.radam_fixture()
    conf, steps = configs[0], int(gd["steps"])
    whole = _Flat(conf, SLICES["two-slices"], guard=True).attach()
    want = [whole.step(s) for s in range(steps)]
    f = _Flat(conf, SLICES["two-slices"], guard=True).attach()
    for s in range(5):
        got = f.step(s)
    f.status[0] = 2
    for s in (5, 6):
        skipped = f.step(s)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(skipped, got))
    assert f.status.cpu().tolist() == [2, 2, 0, 0] and f.opt._step == 7
    f.status.zero_()
    f.opt.rewind(2)
    assert f.opt._step == 5 and all(f.opt.state[q]["step"] == 5 for q in f.params)
    lr = f.opt.param_groups[0]["lr"]
    for s in range(5, steps):
        got = f.step(s)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want[s])), f"step {s + 1}"
    assert f.status.cpu().tolist() == [0, 0, 0, 0] and f.opt.param_groups[0]["lr"] == lr * float(gd["lr_decay"])


# ----------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("overlap", [True, False], ids=["multi-stream", "single-stream"])
def test_engine_optimizer_step_vs_oracle_teacher_forced(overlap):
    """TrainEngine for 8 steps (lr x 0.995 after step 7): before each step the flat p, m, v are copied, after it the flat gradient
    is read, the float64 oracle's step k is applied to the copies, and p, m, v of the WHOLE buffer (25.5 M elements, compared on
    the device) are held to the bound.  No network oracle is needed: this checks the step count, the scalars, lr, and that the
    decoder's early slice (weight-gradient stream, multi-stream schedule) and the remainder cover every element exactly once."""
    case = helpers.ENGINE_CASES[0]
    se, de, st = [m.to(DEV).train() for m in helpers.build_nets()]
    ds = engine.DeviceDataset(helpers.engine_case_data(case), case["window"], torch.device(DEV))
    lr = 1e-4
    eng = engine.TrainEngine(se, de, st, ds, synth.PARENTS, synth.DT, lr=lr, eps=EPS, noise_seed=case["noise_seed"], overlap_wgrads=overlap)
    perm = np.random.default_rng(case["data_seed"]).permutation(len(ds))
    n = eng.flat_p.numel()
    assert n > 8388608 and eng.opt._flat[0] is eng.flat_p and eng.status is not None
    for k in range(1, 9):
        torch.cuda.synchronize()
        before = tuple(t.clone() for t in eng.opt._flat[:1] + eng.opt._flat[2:])
        eng.step(engine.shard_indices(perm, k - 1, case["B"], 1, 0), case["L"])
        torch.cuda.synchronize()
        assert eng.status.cpu().tolist()[:2] == [0, 0], "a sweep gave up: the step was skipped"
        grad = eng.flat_g.clone()
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
        after = (eng.flat_p, eng.opt._flat[2], eng.opt._flat[3])
        _note(helpers.radam_teacher_forced(before, grad, after, k, lr, EPS), f"engine {'multi' if overlap else 'single'}-stream step {k}")
        assert eng.opt._step == k and all(eng.opt.state[q]["step"] == k for q in eng.params[:3])
        if k == 7:
            lr *= 0.995
            for grp in eng.opt.param_groups:
                grp["lr"] = lr
    assert eng.opt.early_pieces == (8 if overlap else 0), eng.opt.early_pieces
    eng.flush()
