"""-m gpu: vote counts under adaptive sampling and the decided-vote stop rule (bmi_forward_mcd_adaptive_votes; MCDEngine.accumulate_adaptive
with V, predict_adaptive(votes=True), ``rule="votes"``) against a fixed run done step by step with ``accumulate_votes(t_begin = k t_step,
t_count = t_step)``: t_used / active_after_step equal a numpy re-derivation of the rule from the V snapshots, every image's S / H / Q / QH
/ V equal the snapshot at its own t_used bit for bit, and — the theorem — with slack 0 every image's majority vote at the tested row is
the full T_max run's.  Integer and bitwise equality throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from bayesnn_fpga_amd.train.uncertainty import vote_decided_numpy, vote_readout_numpy
from tests.helpers import build_seeded
from tests.test_adaptive_ensemble import MODELS
from tests.test_adaptive_sampling import pick_threshold

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
B, T_MAX, T_STEP = 45, 16, 4
CONFIGS = [("r18_block", "f16"), ("r18_block", "f16x2"), ("r18_exit_only_c100", "f16"), ("r18_masksembles", "f16"), ("vgg19", "f16")]
# Per model: the seed of the synthetic weights and the row the rule tests under stop_on "exit" / "ensemble" — chosen so that the images
# retire at more than one step (a condition on the input: synthetic weights vote almost unanimously at most rows, and the four masks of
# the Masksembles model give every image the same split at seed 0)
INPUTS = {"r18_block": (0, 2, 3), "r18_exit_only_c100": (0, 1, 1), "r18_masksembles": (4, 3, 3), "vgg19": (0, 3, 4)}
NAMES = ("S", "H", "Q", "QH", "V")

_ENGINES = {}
_SNAPS = {}


def engine(name, dt, max_batch=B):
    key = (name, dt, max_batch)
    if key not in _ENGINES:
        cls, kw = MODELS[name]
        m = synthetic_weights_(build_seeded(cls, kw), INPUTS[name][0])
        _ENGINES[key] = m.to(DEV).eval().engine(torch.device(DEV), max_batch=max_batch, chunk_samples=T_STEP, dtype=dt)
    return _ENGINES[key]


def snapshots(eng, x, seed, key=None):
    """The fixed run step by step: {t: (S, H, Q, QH, V)} after every step (t = samples so far), on the host.  Computed once per key."""
    if key is not None and key in _SNAPS:
        return _SNAPS[key]
    sums = eng.new_ensemble_sums(x.shape[0])
    V = eng.new_vote_counts(x.shape[0])
    out = {}
    for t0 in range(0, T_MAX, T_STEP):
        eng.accumulate_votes(x, *sums, V, t0, T_STEP, seed, 0)
        out[t0 + T_STEP] = tuple(a.cpu().numpy().copy() for a in (*sums, V))
    if key is not None:
        _SNAPS[key] = out
    return out


def rederive(snap, kind, e, slack, n):
    """t_used / active_after_step of the vote rule applied to the V snapshots"""
    ts = sorted(snap)
    t_used = np.full(n, ts[-1], dtype=np.int32)
    active = np.ones(n, dtype=bool)
    act = []
    for t in ts:
        decided, _ = vote_decided_numpy(snap[t][4][kind, e], t, T_MAX, slack)
        t_used[active] = t
        active &= ~decided
        act.append(int(active.sum()))
        if not active.any():
            break
    return t_used, act + [0] * (len(ts) - len(act))


def run(eng, x, thr, rule, seed, stop_on, test_exit=-1, image_offset=0):
    n = x.shape[0]
    sums = eng.new_ensemble_sums(n)
    S, H, Q, QH = sums
    V = eng.new_vote_counts(n)
    t_used, conv, act = eng.accumulate_adaptive(x, S, T_MAX, thr, rule, T_STEP, test_exit, seed, 0, H, image_offset, ensemble=True,
                                                stop_on=stop_on, Q=Q, QH=QH, V=V)
    return tuple(a.cpu().numpy() for a in (*sums, V)), t_used.cpu().numpy(), conv.cpu().numpy().astype(bool), act


def check_truncation(snap, got, t_used, lo=0):
    for b in range(len(t_used)):
        ref = snap[int(t_used[b])]
        for i, name in enumerate(NAMES):
            g, r = (got[i][:, :, b], ref[i][:, :, lo + b]) if got[i].ndim == 4 else (got[i][:, b], ref[i][:, lo + b])
            np.testing.assert_array_equal(g, r, err_msg=f"{name} of image {b} at t_used={int(t_used[b])}")


@pytest.mark.parametrize("stop_on", ["exit", "ensemble"])
@pytest.mark.parametrize("name,dt", CONFIGS, ids=["/".join(c) for c in CONFIGS])
def test_decided_votes_stop_early_and_keep_the_full_runs_majority(name, dt, stop_on):
    seed = 11
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    kind = _lib.STOP_ON[stop_on]
    e = INPUTS[name][1 + kind]
    got, t_used, conv, act = run(eng, x, 0, "votes", seed, stop_on, test_exit=e)
    want_t, want_act = rederive(snap, kind, e, 0, B)
    print(f"{name}/{dt}/stop_on={stop_on}: active after steps {act}, mean t_used {t_used.mean():.2f}")
    np.testing.assert_array_equal(t_used, want_t)
    assert act == want_act
    check_truncation(snap, got, t_used)
    # the theorem: the majority vote of the truncated run at the tested row is the full run's, for every image
    cls = vote_readout_numpy(got[4][kind, e])["vote_class"]
    np.testing.assert_array_equal(cls, vote_readout_numpy(snap[T_MAX][4][kind, e])["vote_class"])
    assert conv.all()                                  # r = 0 at T_max: the rule holds for every image at its t_used
    assert (got[4][kind, e].sum(-1) == t_used).all()   # every pass of the tested row voted
    assert len(set(t_used.tolist())) >= 2, f"images should retire at more than one step ({act})"


def test_a_slack_of_t_max_retires_everybody_after_the_first_step():
    seed, name, dt = 11, "r18_block", "f16"
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    got, t_used, conv, act = run(eng, x, T_MAX, "votes", seed, "exit")
    assert (t_used == T_STEP).all() and act == [0, 0, 0, 0] and conv.all()
    check_truncation(snap, got, t_used)
    # a slack between: the re-derivation again, and no later than slack 0
    got, t2, conv, act = run(eng, x, 2, "votes", seed, "ensemble")
    want_t, want_act = rederive(snap, 1, eng.n_exits - 1, 2, B)
    np.testing.assert_array_equal(t2, want_t)
    assert act == want_act and conv.all() and (t2 <= rederive(snap, 1, eng.n_exits - 1, 0, B)[0]).all()
    check_truncation(snap, got, t2)


def test_an_inner_row_and_an_image_share():
    seed, name, dt = 11, "r18_block", "f16"
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    got, t_used, conv, act = run(eng, x, 0, "votes", seed, "ensemble", test_exit=1)
    want_t, want_act = rederive(snap, 1, 1, 0, B)
    np.testing.assert_array_equal(t_used, want_t)
    assert act == want_act and conv.all()
    check_truncation(snap, got, t_used)
    cls = vote_readout_numpy(got[4][1, 1])["vote_class"]
    np.testing.assert_array_equal(cls, vote_readout_numpy(snap[T_MAX][4][1, 1])["vote_class"])
    # a share of the batch under image_offset: its rows of the whole batch's run
    off = next(o for o in (16, 32) if eng.image_offset_ok(o))
    whole, tw, _, _ = run(eng, x, 1, "votes", seed, "exit")
    part, tp, cp, _ = run(eng, x[off:off + 13].contiguous(), 1, "votes", seed, "exit", image_offset=off)
    np.testing.assert_array_equal(tp, tw[off:off + 13])
    assert cp.all()
    check_truncation(snap, part, tp, lo=off)


def test_predict_adaptive_reads_the_votes_out():
    seed, name, dt = 11, "r18_exit_only_c100", "f16"
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    r = eng.predict_adaptive(x, T_MAX, 0, rule="votes", t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble", votes=True)
    t_used = r["t_used"].cpu().numpy()
    np.testing.assert_array_equal(t_used, rederive(snap, 1, eng.n_exits - 1, 0, B)[0])
    assert r["converged"].all() and tuple(r["V"].shape) == (2, eng.n_exits, B, eng.out_dim)
    want = vote_readout_numpy(r["V"].cpu().numpy())
    for pre, kind in (("", 0), ("ens_", 1)):
        assert torch.equal(r[pre + "votes"], r["V"][kind])
        assert np.array_equal(r[pre + "vote_class"].cpu().numpy(), want["vote_class"][kind])
        assert np.array_equal(r[pre + "variation_ratio"].cpu().numpy(), want["variation_ratio"][kind])
        np.testing.assert_allclose(r[pre + "vote_entropy"].cpu().numpy(), want["vote_entropy"][kind], rtol=1e-12, atol=0)
    assert (r["V"].sum(-1).cpu().numpy() == t_used[None, None, :]).all()
    for k in ("Q", "QH", "ens_mean", "mean", "pred_entropy"):
        assert k in r
    eng.check_finite()


@pytest.mark.parametrize("stop_on", ["exit", "ensemble"])
def test_a_moment_rule_with_votes_keeps_its_decisions(stop_on):
    """rule="sem" with V: t_used / converged / the sums are accumulate_adaptive(ensemble=True)'s bit for bit, V is the truncated read-out."""
    seed, name, dt = 11, "r18_block", "f16"
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    i = 2 if stop_on == "ensemble" else 0
    thr = pick_threshold({t: (v[i],) for t, v in snap.items()}, eng.n_exits - 1, "sem", 0.4)
    S0, H0, Q0, QH0 = eng.new_ensemble_sums(B)
    t0, c0, act0 = eng.accumulate_adaptive(x, S0, T_MAX, thr, "sem", T_STEP, -1, seed, 0, H0, ensemble=True, stop_on=stop_on, Q=Q0, QH=QH0)
    got, t_used, conv, act = run(eng, x, thr, "sem", seed, stop_on)
    np.testing.assert_array_equal(t_used, t0.cpu().numpy())
    np.testing.assert_array_equal(conv, c0.cpu().numpy().astype(bool))
    assert act == act0 and len(set(t_used.tolist())) >= 2
    for g, w in zip(got, (S0, H0, Q0, QH0)):
        np.testing.assert_array_equal(g, w.cpu().numpy())
    check_truncation(snap, got, t_used)


def test_the_exact_engine_is_refused_and_nothing_is_written():
    x = synthetic_images(8, seed=27).to(DEV)
    exact = engine("r18_block", "f32", max_batch=8)
    S, H, Q, QH = exact.new_ensemble_sums(8)
    V = exact.new_vote_counts(8)
    with pytest.raises(_lib.BmiError) as ei:
        exact.accumulate_adaptive(x, S, 8, 0, "votes", 4, -1, 0, 0, H, ensemble=True, Q=Q, QH=QH, V=V)
    assert ei.value.code == -95                                   # BMI_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not S._base.any() and not V.any()
    # the C ABI on the fp16 engine: a fractional slack, an unknown rule, a null V — nothing written; then the call goes through
    eng = engine("r18_block", "f16", max_batch=8)
    S, H, Q, QH = eng.new_ensemble_sums(8)
    V = eng.new_vote_counts(8)
    need = int(eng.lib.bmi_ensemble_scratch_bytes(eng.handle, 8))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    t_used = torch.zeros(8, dtype=torch.int32, device=DEV)
    conv = torch.zeros(8, dtype=torch.uint8, device=DEV)
    act = (C.c_int32 * 2)()

    def call(rule=2, thr=0.0, v=V.data_ptr(), nbytes=need):
        return eng.lib.bmi_forward_mcd_adaptive_votes(
            eng.handle, x.data_ptr(), 8, 0, 8, 4, 7, 0, rule, thr, eng.n_exits - 1, 1, S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
            H.data_ptr(), Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), v, None, scratch.data_ptr(), nbytes, t_used.data_ptr(),
            conv.data_ptr(), act, eng.workspace.data_ptr(), eng.workspace_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(thr=0.5) == -22 and call(rule=3) == -22 and call(v=None) == -22 and call(nbytes=need - 1) == -12
    torch.cuda.synchronize()
    assert not S._base.any() and not V.any() and not t_used.any() and not conv.any() and list(act) == [0, 0]
    assert call() == 0
    torch.cuda.synchronize()
    assert V.any() and (t_used > 0).all() and conv.all()
