"""Held-out evaluation on the device: the forward-only, per-window loss kernel (zeggs_loss_eval, csrc/loss.hip) against the
float64 oracle of tests/eval_helpers.py, its row independence (bitwise), its agreement with the training kernel, the group
accumulation (zeggs_eval_accumulate), the refusals, and zeggs.evaluate.evaluate() end to end, beside a training engine and
inside train().

Bounds: none new.  Every column is held to helpers.LOSS_TERM_BOUND (rtol 3e-5, atol 1e-7), the bound the training kernel's terms
meet at B = 1 -- a window here is such a batch, and the sums run in float64.  Against the training kernel: twice that bound
(each side is within it of the exact value); the KL to helpers.LOSS_KL_BOUND.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import eval_helpers
import helpers
from oracle import loss as oloss
from zeggs import engine, evaluate, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KLW = oloss.kl_weight(helpers.LOSS_KL_ITERATION)
DIFF = list(oloss.DIFF_TERMS)
_ORACLE = {}


class _lds:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        ops.set_option("loss_lds", self.v)

    def __exit__(self, *exc):
        ops.set_option("loss_lds", 1)
        return False


def _rows(d, kl=True):
    """ops.loss_eval on a case -> float64 [B, 22] on the host"""
    a = eval_helpers.device_inputs(d, DEV)
    mu, lv = (d["mu"].to(DEV), d["logvar"].to(DEV)) if kl else (None, None)
    rows = ops.loss_eval(*a[:7], a[7], synth.DT, mu, lv)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float64 and rows.shape == (d["O"][0].shape[0], ops.EVAL_COLS)
    return rows.cpu()


def _oracle(case):
    key = helpers.loss_case_id(case)
    if key not in _ORACLE:
        d = helpers.loss_case(case)
        _ORACLE[key] = (d, eval_helpers.rows_oracle(d))
    return _ORACLE[key]


# ----------------------------------------------------------------------------- 1. the kernel against float64, per window
@pytest.mark.parametrize("loss_lds", [1, 0])
@pytest.mark.parametrize("case", eval_helpers.EVAL_CASES, ids=helpers.loss_case_id)
def test_rows_vs_oracle(case, loss_lds):
    d, ref = _oracle(case)
    with _lds(loss_lds):
        got = _rows(d)
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-300))
    err[ref == 0] = 0
    print(f"\nMEASURED {helpers.loss_case_id(case)} loss_lds={loss_lds} terms={float(err[:, :17].max()):.1e} "
          + " ".join(f"c{c}={float(err[:, c].max()):.1e}" for c in range(17, 22)))
    assert torch.isfinite(got).all()
    if d["T"] == 1:
        assert float(got[:, DIFF].abs().max()) == 0.0
    np.testing.assert_allclose(got.numpy(), ref.numpy(), err_msg=helpers.loss_case_id(case), **helpers.LOSS_TERM_BOUND)


def test_workspace_is_no_larger_than_the_training_call():
    L = ops.lib()
    for case in eval_helpers.EVAL_CASES + [("rig", 32, 256, "general"), ("j1", 1, 1, "general")]:
        d = ops.LossDims(case[1], case[2], len(helpers.LOSS_SKELETONS[case[0]]), 64, synth.DT)
        assert 0 < L.zeggs_loss_eval_workspace_bytes(C.byref(d)) <= L.zeggs_loss_workspace_bytes(C.byref(d)), case


# ----------------------------------------------------------------------------- 2. windows are independent, bitwise
def test_rows_are_independent_bitwise():
    d = helpers.loss_case(("rig", 5, 28, "general"))
    base = _rows(d)
    assert torch.equal(base, _rows(d))                                      # call to call
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(_rows(eval_helpers.permuted(d, perm)), base[perm])
    one = _rows(eval_helpers.with_row_as_truth(d, 2))
    assert float(one[2, :20].abs().max()) == 0.0
    assert float(one[2, 20]) == float(one[2, 21]) > 0
    keep = [0, 1, 3, 4]
    assert torch.equal(one[keep], base[keep])
    assert float(base[:, :20].min()) > 0
    nokl = _rows(d, kl=False)                                               # mu == NULL: column 17 is 0, the rest unchanged
    assert float(nokl[:, 17].abs().max()) == 0.0
    cols = [c for c in range(22) if c != 17]
    assert torch.equal(nokl[:, cols], base[:, cols])


# ----------------------------------------------------------------------------- 3. agreement with the training kernel
@pytest.mark.parametrize("B,T", [(3, 7), (2, 8)])
def test_mean_of_rows_is_the_training_loss(B, T):
    d = helpers.loss_case(("rig", B, T, "general"))
    a = eval_helpers.device_inputs(d, DEV)
    mu, lv = d["mu"].to(DEV), d["logvar"].to(DEV)
    _, terms = ops.training_loss(*a[:7], a[7], synth.DT, mu, lv, kl_weight=KLW)
    rows = _rows(d)
    terms = terms.cpu().double()
    np.testing.assert_allclose(rows[:, :17].mean(0).numpy(), terms[:17].numpy(), rtol=2 * helpers.LOSS_TERM_BOUND["rtol"],
                               atol=2 * helpers.LOSS_TERM_BOUND["atol"])
    kl = KLW * float(rows[:, 17].mean())
    assert abs(kl - float(terms[17])) <= helpers.LOSS_KL_BOUND * abs(float(terms[17])), (kl, float(terms[17]))


# ----------------------------------------------------------------------------- 4. zeggs_eval_accumulate
def test_accumulate_is_the_host_sum_in_row_order():
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((7, 22)) * 10.0 ** rng.integers(-6, 6, (7, 22))
    group = [0, 2, -1, 2, 1, -1, 0]
    want = np.zeros((3, 23))
    want[:, :22] = rng.standard_normal((3, 22))          # acc is added to, not overwritten
    acc = torch.as_tensor(want.copy()).to(DEV)
    for b, g in enumerate(group):
        if g >= 0:
            want[g, :22] += rows[b]
            want[g, 22] += 1
    ops.eval_accumulate(torch.as_tensor(rows).to(DEV), torch.as_tensor(group, dtype=torch.int32).to(DEV), acc)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert np.array_equal(got, want)
    assert got[:, 22].tolist() == [2, 1, 2]


# ----------------------------------------------------------------------------- 5. refusals
def test_bad_arguments_are_refused_before_any_launch():
    L = ops.lib()
    d = helpers.loss_case(("rig", 2, 8, "general"))
    a = eval_helpers.device_inputs(d, DEV)
    rows = torch.full((2, 22), 7.0, device=DEV, dtype=torch.float64)
    ws = torch.zeros(int(L.zeggs_loss_workspace_bytes(C.byref(ops.LossDims(2, 8, 257, 0, synth.DT)))), dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(dims, nbytes):
        return L.zeggs_loss_eval(C.byref(dims), p(a[7]), p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), p(a[6]), None, None,
                                 p(rows), p(ws), C.c_size_t(nbytes), stream)
    assert call(ops.LossDims(2, 8, 257, 0, synth.DT), ws.numel()) == -1
    assert "256" in L.zeggs_last_error().decode()
    good = ops.LossDims(2, 8, 75, 0, synth.DT)
    need = int(L.zeggs_loss_eval_workspace_bytes(C.byref(good)))
    assert call(good, need - 1) == -1
    assert "workspace" in L.zeggs_last_error().decode()
    assert call(ops.LossDims(0, 8, 75, 0, synth.DT), ws.numel()) == -1
    torch.cuda.synchronize()
    assert float(rows.min()) == 7.0 == float(rows.max()) and int(ws.max()) == 0          # nothing was launched
    assert call(good, need) == 0                                                         # ... and the exact size is accepted
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu(), _rows(d, kl=False))


# ----------------------------------------------------------------------------- 6. evaluate() end to end
def _nets():
    se, de, st = helpers.build_nets()
    return se.to(DEV).eval(), de.to(DEV).eval(), st.to(DEV).eval()


def _expected_table(data, nets, window, batch, example_len, nlabels):
    """Per-label sums built from the code the training step runs: the batches of the plan gathered by DeviceDataset.batch of a
    dataset whose TRAINING ranges are the validation ranges, the networks as TrainEngine.step calls them at B = batch, then
    ops.training_loss on every real row alone."""
    se, de, st = nets
    twin = dict(data)
    twin["ranges_train"], twin["ranges_train_labels"] = data["ranges_valid"], data["ranges_valid_labels"]
    ds = engine.DeviceDataset(twin, window, torch.device(DEV))
    starts, ridx = evaluate.plan_windows(data["ranges_valid"], window)
    where = {int(s): i for i, s in enumerate(ds.win_start)}
    parents = torch.as_tensor(synth.PARENTS, dtype=torch.int32, device=DEV)
    table = np.zeros((nlabels, 23))
    with torch.no_grad():
        for b0 in range(0, len(starts), batch):
            real = list(range(b0, min(b0 + batch, len(starts))))
            rows = real + [b0] * (batch - len(real))                       # padded with copies of the batch's first window
            b = ds.batch(np.asarray([where[int(starts[r])] for r in rows]), example_len, style_encoder=st.encoder)
            speech = se(b["audio"])
            z, mu, logvar = st(b["example"], 1.0, eps=torch.zeros(batch, 64, device=DEV))
            style = ops.broadcast_time(z, window)
            pose, rpos, rrot = ops.decoder_core(de, b["pose0"], b["rpos0"], b["rrot0"], b["gaze"], speech, style, ds.in_mean,
                                                ds.in_std, ds.out_mean, ds.out_std, synth.DT)
            for k, r in enumerate(real):
                s = slice(k, k + 1)
                _, terms = ops.training_loss(pose[s], rpos[s], rrot[s], b["pose"][s], b["rpos"][s], b["rrot"][s], b["gaze"][s],
                                             parents, synth.DT, mu[s], logvar[s], kl_weight=KLW)
                g = int(data["ranges_valid_labels"][ridx[r]])
                table[g, :18] += terms[:18].cpu().double().numpy()
                table[g, 22] += 1
    return table


def test_evaluate_end_to_end():
    window, batch, L = 8, 4, 16
    data = synth.make_processed(2, 3, 21, seed=17)
    nets = _nets()
    ds = engine.DeviceDataset(data, window, torch.device(DEV))
    kw = dict(split="valid", batch=batch, example_len=L, iteration=helpers.LOSS_KL_ITERATION)
    res = evaluate.evaluate(*nets, ds, synth.PARENTS, synth.DT, **kw)
    want = _expected_table(data, nets, window, batch, L, res["table"].shape[0])
    assert res["windows"] == 6 and res["frames_scored"] == 48 and res["frames_total"] == 63
    labels = np.asarray(data["ranges_valid_labels"])
    counts = {int(g): 2 * int((labels == g).sum()) for g in set(labels.tolist())}     # two windows per range: the padded rows are not in
    assert {g: r["windows"] for g, r in res["per_label"].items()} == counts
    assert res["table"][:, 22].sum() == 6 and np.array_equal(res["table"][:, 22], want[:, 22])
    from zeggs.train import LOSS_TAGS
    tol = dict(rtol=2 * helpers.LOSS_TERM_BOUND["rtol"], atol=2 * helpers.LOSS_TERM_BOUND["atol"])
    np.testing.assert_allclose([res["terms"][t] for t in LOSS_TAGS[:17]], want[:, :17].sum(0) / 6, **tol)
    for g, r in res["per_label"].items():
        np.testing.assert_allclose([r["terms"][t] for t in LOSS_TAGS[:17]], want[g, :17] / want[g, 22], **tol)
    kl = want[:, 17].sum() / 6
    assert abs(res["terms"]["loss_kl_div"] - kl) <= helpers.LOSS_KL_BOUND * abs(kl)
    assert abs(res["loss"] - want[:, :18].sum() / 6 / 18) <= 2 * helpers.LOSS_BOUND * abs(res["loss"])
    assert all(np.isfinite(res[k]) and res[k] > 0 for k in ("mpjpe", "root_drift", "speed_pred", "speed_true"))
    # max_windows, the training split
    assert evaluate.evaluate(*nets, ds, synth.PARENTS, synth.DT, max_windows=3, **kw)["windows"] == 3
    tr = evaluate.evaluate(*nets, ds, synth.PARENTS, synth.DT, **dict(kw, split="train"))
    assert tr["windows"] == 4 and tr["frames_total"] == 42 and np.isfinite(tr["loss"])
    assert all(not m.training for m in nets)


def test_two_ranks_sum_to_the_single_rank_table():
    """reduce=False tables of world = 2, ranks 0 and 1 (one batch each), against the world = 1 table at rtol 1e-12.  Holds because
    evaluate() runs the networks' products in a fixed summation order (ops.fixed_order_gemms): with the split-K atomics of the
    training routing the same windows differed by 1.2e-7 .. 2.4e-7 relative from call to call; with the fixed order the measured
    difference is 0."""
    window, batch, L = 8, 4, 16
    nets = _nets()
    ds = engine.DeviceDataset(synth.make_processed(2, 3, 21, seed=17), window, torch.device(DEV))
    kw = dict(split="valid", batch=batch, example_len=L, iteration=helpers.LOSS_KL_ITERATION)
    whole = evaluate.evaluate(*nets, ds, synth.PARENTS, synth.DT, **kw)["table"]
    parts = [evaluate.evaluate(*nets, ds, synth.PARENTS, synth.DT, world=2, rank=r, reduce=False, **kw) for r in (0, 1)]
    assert [int(p[:, 22].sum()) for p in parts] == [4, 2]
    assert np.array_equal((parts[0] + parts[1])[:, 22], whole[:, 22])
    rel = np.abs(parts[0] + parts[1] - whole) / np.maximum(np.abs(whole), 1e-300)
    print(f"\nMEASURED two ranks against one: max relative difference {rel.max():.2e}")
    np.testing.assert_allclose(parts[0] + parts[1], whole, rtol=1e-12, atol=0)


def test_evaluate_counts_no_splitting_route_and_the_same_forward_outside_does():
    """What the two-rank test above rests on, shown not to be vacuous at its shape (window 8, batch 4, example 16): on the calling
    thread's route log (ops.gemm_route_log) evaluate() launches products, none of them on a route that splits its contraction --
    and ONE forward of the same networks on a batch of the same shape outside the block does take splitting routes (measured: the
    mid-split once and the LDS-tiled stream-K kernel twice, in the style encoder), so without the fixed order the scores would
    carry the atomics' call-to-call rounding.  The shape did not have to be enlarged."""
    window, batch, L = 8, 4, 16
    data = synth.make_processed(2, 3, 21, seed=17)
    se, de, st = nets = _nets()
    ds = engine.DeviceDataset(data, window, torch.device(DEV))
    splitting = set(ops.GEMM_SPLITTING_ROUTES)
    ops.gemm_route_log(reset=True)
    evaluate.evaluate(*nets, ds, synth.PARENTS, synth.DT, split="valid", batch=batch, example_len=L, iteration=helpers.LOSS_KL_ITERATION)
    inside = ops.gemm_route_log(reset=True)["counts"]
    assert sum(inside.values()) > 0 and not splitting & set(inside), inside
    twin = dict(data)
    twin["ranges_train"], twin["ranges_train_labels"] = data["ranges_valid"], data["ranges_valid_labels"]
    tds = engine.DeviceDataset(twin, window, torch.device(DEV))
    with torch.no_grad():
        b = tds.batch(np.arange(batch), L, style_encoder=st.encoder)
        ops.gemm_route_log(reset=True)
        speech = se(b["audio"])
        z, _, _ = st(b["example"], 1.0, eps=torch.zeros(batch, 64, device=DEV))
        ops.decoder_core(de, b["pose0"], b["rpos0"], b["rrot0"], b["gaze"], speech, ops.broadcast_time(z, window), tds.in_mean,
                         tds.in_std, tds.out_mean, tds.out_std, synth.DT)
    torch.cuda.synchronize()
    outside = ops.gemm_route_log(reset=True)["counts"]
    print(f"\nMEASURED routes inside evaluate(): {inside}; one forward outside: {outside}")
    assert splitting & set(outside), outside
    assert ops.lib().zeggs_gemm_fixed_order(0) == 0           # evaluate() left the thread as it found it


def test_evaluate_empty_split():
    ds = engine.DeviceDataset(synth.make_processed(2, 0, 21, seed=17), 8, torch.device(DEV))
    res = evaluate.evaluate(*_nets(), ds, synth.PARENTS, synth.DT, batch=4, example_len=16)
    assert res["windows"] == 0 and res["frames_scored"] == 0 and np.isnan(res["loss"]) and res["per_label"] == {}
    short = engine.DeviceDataset(synth.make_processed(2, 1, 8, seed=17), 8, torch.device(DEV))      # a range of `window` frames: no window
    assert evaluate.evaluate(*_nets(), short, synth.PARENTS, synth.DT, batch=4, example_len=16)["windows"] == 0


# ----------------------------------------------------------------------------- 7. evaluation beside a training engine
def test_evaluation_does_not_disturb_training():
    """The recipe of test_gpu_streams.py::test_two_engines_on_two_threads_are_isolated (B 4, T 12, L 16, the persistent sweeps off,
    6 steps, training mode): with the next batch prefetched, the engine flushed and the validation split scored behind steps 2 and
    4, the weights end within that test's run-to-run bound of the plain run's."""
    import copy
    B, T, L, steps = 4, 12, 16, 6
    dev = torch.device(DEV)

    def run(with_eval):
        se, de, st = helpers.build_nets(seed=1234)
        se, de, st = se.to(dev).train(), de.to(dev).train(), st.to(dev).train()
        ds = engine.DeviceDataset(synth.make_processed(3, 2, T + 40, seed=21), T, dev)
        eng = engine.TrainEngine(se, de, st, ds, synth.PARENTS, synth.DT, noise_seed=11)
        perm = np.random.default_rng(1234).permutation(len(ds))
        results = []
        for k in range(steps):
            eng.step(engine.shard_indices(perm, k, B, 1, 0), L)
            if with_eval and k in (2, 4):
                eng.prefetch(engine.shard_indices(perm, k + 1, B, 1, 0), L)
                eng.flush()
                before = (copy.deepcopy(eng.ctx.rng().bit_generator.state), copy.deepcopy(ops._seed_rng.bit_generator.state))
                results.append(evaluate.evaluate(se, de, st, ds, synth.PARENTS, synth.DT, batch=B, example_len=L, iteration=k))
                assert (eng.ctx.rng().bit_generator.state, ops._seed_rng.bit_generator.state) == before
                assert se.training and de.training and st.training
                assert eng._prefetched is not None
        torch.cuda.synchronize()
        eng.flush()
        if with_eval:
            assert eng.prefetch_hits == 2
            assert all(r["windows"] == 8 and np.isfinite(r["loss"]) for r in results), results
        return eng.flat_p.detach().cpu().numpy().copy()

    saved = {k: ops._OPTIONS.get(k, 1) for k in ("train_persistent", "bwd_persistent")}
    for k in saved:
        ops.set_option(k, 0)
    try:
        plain, scored = run(False), run(True)
    finally:
        for k, v in saved.items():
            ops.set_option(k, v)
    assert np.isfinite(scored).all()
    assert np.abs(scored - plain).max() <= 2e-6, np.abs(scored - plain).max()


def test_training_flags_are_restored_after_an_error():
    class Broken(torch.nn.Module):
        def forward(self, x):
            raise RuntimeError("no speech encoder today")
    _, de, st = _nets()
    se = Broken().train()
    st.train()
    ds = engine.DeviceDataset(synth.make_processed(2, 1, 21, seed=17), 8, torch.device(DEV))
    with pytest.raises(RuntimeError, match="no speech encoder today"):
        evaluate.evaluate(se, de, st, ds, synth.PARENTS, synth.DT, batch=4, example_len=16)
    assert se.training and not de.training and st.training


# ----------------------------------------------------------------------------- 8. train() and the command line
NET_OPT = {"decoder": {"nhidden": 1024, "num_rnn_layers": 2, "rnn_cond": "normal"},
           "speech_encoder": {"nhidden": 64, "speech_encoding_size": 64},
           "style_encoder": {"nhidden": 512, "style_encoding_size": 64, "example_length": 16, "type": "attn", "use_vae": True}}
TRAIN_OPT = dict(niterations=0.004, batchsize=4, window=8, change_pace=True, learning_rate=1e-4, learning_rate_decay=0.995,
                 eps=1e-5, resume=False, use_gpu=True, thread_count=1, seed=1234, use_tensorboard=True,
                 style_encoding_type="example", generate_samples_step=5, use_script=False)


def _eval_csv(path):
    import csv
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def test_train_writes_eval_csv_and_cli_evaluate(tmp_path, capsys):
    from zeggs import cli
    from zeggs import train as train_mod
    synth.write_dataset(tmp_path / "data", n_train=1, n_valid=1, nframes=32, seed=3)       # 24 windows: 6 iterations per epoch
    options = {"paths": {"base_path": str(tmp_path), "path_processed_data": "data", "output_dir": str(tmp_path / "run"),
                         "models_dir": None},
               "net_opt": NET_OPT, "train_opt": dict(TRAIN_OPT, eval_every=2)}
    (tmp_path / "options.json").write_text(json.dumps(options))
    assert cli.main(["train", "-o", str(tmp_path / "options.json")]) == 0
    n = train_mod.last_engine.iteration
    rows = _eval_csv(tmp_path / "run" / "logs" / "eval.csv")
    assert [int(r["iteration"]) for r in rows] == sorted({i for i in range(n) if i % 2 == 0 or i % 5 == 0})
    assert all(int(r["windows"]) == 3 and int(r["frames_scored"]) == 24 and int(r["frames_total"]) == 32 for r in rows)
    assert all(np.isfinite(float(v)) for r in rows for v in r.values())
    assert set(train_mod.LOSS_TAGS) <= set(rows[0]) and float(rows[0]["mpjpe"]) > 0
    if (tmp_path / "run" / "logs" / "tb" / "scalars.jsonl").exists():      # no tensorboard package: the JSON-lines twin
        logged = [json.loads(x) for x in open(tmp_path / "run" / "logs" / "tb" / "valid_scalars.jsonl")]
        assert [x["iteration"] for x in logged] == [int(r["iteration"]) for r in rows]
        assert all(set(x) >= {"valid/total_loss", "valid/losses", "valid/mpjpe"} for x in logged)
        assert len(open(tmp_path / "run" / "logs" / "tb" / "scalars.jsonl").readlines()) == n
    # the same run without the key: the checkpoint iterations only
    (tmp_path / "m2").mkdir(), (tmp_path / "l2").mkdir()
    train_mod.train(tmp_path / "m2", tmp_path / "l2", tmp_path / "data" / "processed_data.npz",
                    tmp_path / "data" / "data_definition.json", dict(TRAIN_OPT), NET_OPT)
    rows2 = _eval_csv(tmp_path / "l2" / "eval.csv")
    assert [int(r["iteration"]) for r in rows2] == [i for i in range(train_mod.last_engine.iteration) if i % 5 == 0]
    # the command line on the first run's checkpoints
    capsys.readouterr()
    out_json = tmp_path / "scores.json"
    assert cli.main(["evaluate", "-o", str(tmp_path / "run" / "options.json"), "--batch", "2", "--json", str(out_json)]) == 0
    text = capsys.readouterr().out
    assert "label" in text and "mpjpe" in text and "all" in text
    res = json.loads(out_json.read_text())
    assert res["windows"] == 3 and res["split"] == "valid" and len(res["per_label"]) == 1
    assert next(iter(res["per_label"])) in synth.LABEL_NAMES and np.isfinite(res["loss"])
    assert cli.main(["evaluate", "-o", str(tmp_path / "run" / "options.json"), "--split", "train", "--max-windows", "2",
                     "--json", str(out_json)]) == 0
    assert json.loads(out_json.read_text())["windows"] == 2
