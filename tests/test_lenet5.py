"""MC-dropout LeNet-5 on the device (csrc/lenet5.hip behind ``engine.LeNet5Engine``) against a plain float64 torch forward of its six
layers with the masks of ``oracle.philox``; for num_bayes_layer = 1 also against ``oracle.mcd.mcd_predict(oracle.extra_models.LeNet5MC)``.
Tolerances are the project's (tests/test_extra_models.py, BASELINE.json): 5e-3 * max(1, max|logit|) on logits, 1e-3 on mean and variance;
a CPU emulation of the kernel's arithmetic (P1 and conv2's operands in fp16, fp32 accumulation) on these inputs stays below 8.9e-3 on
logits of magnitude 22-40, 2.3e-4 on the mean and 1.8e-4 on the variance."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from oracle import extra_models as ox
from oracle import mcd, philox
from tests.helpers import build_seeded

pytestmark = pytest.mark.gpu
T, SEED = 10, 77


def mirror(k, p, out_dim=10):
    return synthetic_weights_(build_seeded(bx.LeNet5MC, dict(num_bayes_layer=k, dropout_p=p, out_dim=out_dim)), 0)


@functools.lru_cache(maxsize=None)
def reference(k, p, B, out_dim=10, n_samples=T):
    """float64 logits [T, 1, B, C], mean and variance [1, B, C] of samples 0 .. T-1."""
    w = {n: v.double() for n, v in mirror(k, p, out_dim).state_dict().items()}
    x = synthetic_images(B, 1234, channels=1, size=28).double()
    on = [loc >= 3 - k for loc in range(3)]
    ids = np.cumsum(on) - 1

    def site(v, loc, t):
        if not on[loc]:
            return v
        return v * torch.from_numpy(philox.elementwise_mask(v.shape, SEED, int(ids[loc]), t, p)).double() * float(philox.drop_scale(p))

    p1 = F.max_pool2d(F.relu(F.conv2d(x, w["conv1.weight"], w["conv1.bias"], padding=2)), 2)
    logits = []
    for t in range(n_samples):
        f = F.max_pool2d(F.relu(F.conv2d(site(p1, 0, t), w["conv2.weight"], w["conv2.bias"], padding=2)), 7).flatten(1)
        h = F.relu(F.linear(site(f, 1, t), w["fc1.weight"], w["fc1.bias"]))
        logits.append(F.linear(site(h, 2, t), w["fc2.weight"], w["fc2.bias"]))
    logits = torch.stack(logits)[:, None]
    probs = torch.softmax(logits, -1)
    return logits.numpy(), probs.mean(0).numpy(), probs.var(0, unbiased=False).numpy()


def run(k, p, B, out_dim=10, n_samples=T):
    m = mirror(k, p, out_dim).to("cuda:0").eval()
    x = synthetic_images(B, 1234, channels=1, size=28).to("cuda:0")
    eng = m.engine(x.device, max_batch=B)
    return m, x, eng, eng.forward_samples(x, n_samples, seed=SEED).cpu().numpy(), {n: v.cpu().numpy() for n, v in eng.predict(x, n_samples, seed=SEED).items()}


def assert_close(logits, r, want):
    for name, got, ref, tol in (("logits", logits, want[0], 5e-3 * max(1.0, float(np.abs(want[0]).max()))), ("mean", r["mean"], want[1], 1e-3),
                                ("var", r["var"], want[2], 1e-3)):
        print(f"{name}: max |error| {np.abs(got - ref).max():.3e} (tolerance {tol:.1e})")
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol, err_msg=name)


# (B, T): at B = 1 and 7 every sample is a workgroup of its own (csrc/lenet5.hip:lenet5_chunks); B = 260 runs ONE chunk whose workgroups loop
# over all four samples in the kernel and add straight into S
@pytest.mark.parametrize("B,n", [(1, T), (7, T), (260, 4)])
@pytest.mark.parametrize("p", [0.25, 0.2])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_parity_with_the_float64_reference(k, p, B, n):
    _, _, _, logits, r = run(k, p, B, n_samples=n)
    assert_close(logits, r, reference(k, p, B, n_samples=n))
    if k == 1:
        o = synthetic_weights_(build_seeded(ox.LeNet5MC, dict(dropout_p=p, out_dim=10)), 0)
        ref = mcd.mcd_predict(o, synthetic_images(B, 1234, channels=1, size=28), n, SEED)
        assert_close(logits, r, (ref["logits"], ref["mean"], ref["var"]))


@pytest.mark.parametrize("B,n", [(260, 4), (130, 10)])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_sample_loop_gives_the_rows_of_single_sample_calls(k, B, n):
    """One chunk of 4 samples (B = 260) and chunks of 4, 4 and 2 samples joined by the second launch (B = 130): every row equals, bit for
    bit, the call that runs that sample alone as the first iteration of its workgroup, and the sums are those of the single-sample calls
    up to the order of the float64 additions."""
    _, x, eng, logits, r = run(k, 0.2, B, n_samples=n)
    S = eng.new_moments(B)
    for t in range(n):
        assert np.array_equal(eng.forward_samples(x, 1, seed=SEED, t_begin=t).cpu().numpy()[0], logits[t]), t
        eng.accumulate(x, S, t, 1, SEED)
    one = eng.finalize(S, n)
    for name in ("mean", "var", "logit_mean"):
        np.testing.assert_allclose(one[name].cpu().numpy(), r[name], rtol=0, atol=1e-12)


def test_sample_addressing():
    m, x, eng, logits, r = run(3, 0.2, 7)
    assert np.array_equal(eng.forward_samples(x, 4, seed=SEED, t_begin=6).cpu().numpy(), logits[6:])
    S = eng.new_moments(7)
    eng.accumulate(x, S, 0, 4, SEED)
    eng.accumulate(x, S, 4, 6, SEED)
    two = eng.finalize(S, T)
    for name in ("mean", "var"):          # the float64 sums only change their order
        np.testing.assert_allclose(two[name].cpu().numpy(), r[name], rtol=0, atol=1e-12)
    m.mc_seed = SEED
    passes = np.stack([m(x)[0].cpu().numpy() for _ in range(T)])
    assert np.array_equal(passes, logits[:, 0]) and m.mc_pass == T


@pytest.mark.parametrize("k,p,out_dim,B", [(3, 0.0, 10, 1), (0, 0.2, 10, 1), (3, 0.2, 3, 1), (3, 0.0, 10, 520), (0, 0.2, 10, 520)])
def test_edges(k, p, out_dim, B):
    """p = 0 at every site and no site at all: every sample is the same, so the raw sums obey S2 * T == S1^2 exactly at T = 8 (sums of 8
    equal fp32 values and of their squares are exact in float64), and the variance is exactly 0 (1 / T is exact; the identity on the raw
    sums is the sharper statement: ``bmi_finalize`` clamps a negative variance to 0).  B = 520: one chunk, all eight samples inside the
    kernel's loop.  Three classes: lanes 3 .. 31 of the softmax wave carry nothing."""
    _, x, eng, logits, r = run(k, p, B, out_dim, 8)
    if B == 1:
        assert_close(logits, r, reference(k, p, 1, out_dim, 8))
    if k == 0 or p == 0.0:
        S = eng.accumulate(x, eng.new_moments(B), 0, 8, SEED)
        assert np.array_equal(logits, np.broadcast_to(logits[:1], logits.shape))
        assert torch.equal(S[1] * 8, S[0] * S[0]) and np.all(r["var"] == 0)
