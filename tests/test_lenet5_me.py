"""Multi-exit MC-dropout LeNet-5 on the device (csrc/lenet5_me.hip behind ``engine.LeNet5Engine``) against a plain float64 torch forward
of its layers with the masks of ``oracle.philox``.  Tolerances are the project's (tests/test_lenet5.py, BASELINE.json): 5e-3 * max(1,
max|logit|) on logits, 1e-3 on mean and variance; a CPU emulation of the kernel's arithmetic (P1 and both convs' operands in fp16, fp32
accumulation) on these inputs stays below 3.9e-3 on the early exit's logits (magnitude 3.4-13, checked against that exit's own magnitude:
tolerance 1.7e-2 or more) and 5.5e-3 on the main exit's (magnitude 13-23), 4.1e-4 on the mean and 1.2e-4 on the variance."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from oracle import philox
from tests.helpers import build_seeded

pytestmark = pytest.mark.gpu
SEED = 77


def mirror(dropout_exit=True, p=0.2, out_dim=10):
    return synthetic_weights_(build_seeded(bx.LeNet5MCEarlyExit, dict(dropout_exit=dropout_exit, dropout_p=p, out_dim=out_dim)), 0)


def forward64(m, x, n_samples):
    """float64 logits [T, 2, B, C] (early exit, main exit), mean and variance [2, B, C] of samples 0 .. T-1."""
    w = {n: v.double() for n, v in m.state_dict().items()}

    def site(v, sid, t):
        if not m.dropout_exit:
            return v
        return v * torch.from_numpy(philox.elementwise_mask(v.shape, SEED, sid, t, m.dropout_p)).double() * float(philox.drop_scale(m.dropout_p))

    p1 = F.max_pool2d(F.relu(F.conv2d(x.double(), w["conv1.weight"], w["conv1.bias"], padding=2)), 2)
    he = F.relu(F.linear(F.relu(F.conv2d(p1, w["ex1conv1.weight"], w["ex1conv1.bias"], stride=7)).flatten(1), w["ex1fc1.weight"], w["ex1fc1.bias"]))
    f = F.max_pool2d(F.relu(F.conv2d(p1, w["conv2.weight"], w["conv2.bias"], padding=2)), 7).flatten(1)
    hm = F.relu(F.linear(f, w["fc1.weight"], w["fc1.bias"]))
    logits = torch.stack([torch.stack([F.linear(site(he, 0, t), w["ex1linear.weight"], w["ex1linear.bias"]),
                                       F.linear(site(hm, 1, t), w["fc2.weight"], w["fc2.bias"])]) for t in range(n_samples)])
    probs = torch.softmax(logits, -1)
    return logits.numpy(), probs.mean(0).numpy(), probs.var(0, unbiased=False).numpy()


@functools.lru_cache(maxsize=None)
def reference(dropout_exit, p, B, out_dim, n_samples):
    return forward64(mirror(dropout_exit, p, out_dim), synthetic_images(B, 1234, channels=1, size=28), n_samples)


def run(m, x, n_samples):
    m, x = m.to("cuda:0").eval(), x.to("cuda:0")
    eng = m.engine(x.device, max_batch=x.shape[0])
    return m, x, eng, eng.forward_samples(x, n_samples, seed=SEED).cpu().numpy(), {n: v.cpu().numpy() for n, v in eng.predict(x, n_samples, seed=SEED).items()}


def assert_close(logits, r, want):
    assert logits.shape == want[0].shape and r["mean"].shape == want[1].shape
    for e in range(2):      # an exit's logits against that exit's own magnitude
        tol = 5e-3 * max(1.0, float(np.abs(want[0][:, e]).max()))
        print(f"exit {e} logits: max |error| {np.abs(logits[:, e] - want[0][:, e]).max():.3e} (tolerance {tol:.1e})")
        np.testing.assert_allclose(logits[:, e], want[0][:, e], rtol=0, atol=tol, err_msg=f"logits of exit {e}")
    for name, got, ref in (("mean", r["mean"], want[1]), ("var", r["var"], want[2])):
        print(f"{name}: max |error| {np.abs(got - ref).max():.3e} (tolerance 1.0e-03)")
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3, err_msg=name)


# B = 3 and 8 hold images whose first keep byte starts four elements early; T = 1, 5, 10: empty, odd and even shares of the waves
@pytest.mark.parametrize("B,n", [(1, 1), (3, 5), (8, 10)])
@pytest.mark.parametrize("p", [0.25, 0.2])
def test_parity_with_the_float64_reference(p, B, n):
    _, _, _, logits, r = run(mirror(True, p), synthetic_images(B, 1234, channels=1, size=28), n)
    assert_close(logits, r, reference(True, p, B, 10, n))


def test_sample_addressing():
    m, x, eng, logits, r = run(mirror(), synthetic_images(3, 1234, channels=1, size=28), 10)
    assert np.array_equal(eng.forward_samples(x, 4, seed=SEED, t_begin=5).cpu().numpy(), logits[5:9])      # every sample on the other wave
    for t in range(10):
        assert np.array_equal(eng.forward_samples(x, 1, seed=SEED, t_begin=t).cpu().numpy()[0], logits[t]), t
    two = eng.finalize(eng.accumulate(x, eng.accumulate(x, eng.new_moments(3), 0, 3, SEED), 3, 7, SEED), 10)
    for name in ("mean", "var"):          # the float64 sums only change their order
        np.testing.assert_allclose(two[name].cpu().numpy(), r[name], rtol=0, atol=1e-12)
    m.mc_seed = SEED
    passes = np.stack([np.stack([o.cpu().numpy() for o in m(x)]) for _ in range(10)])
    assert np.array_equal(passes, logits) and m.mc_pass == 10


@pytest.mark.parametrize("dropout_exit,p,out_dim,B", [(False, 0.2, 10, 1), (True, 0.0, 10, 5), (True, 0.2, 2, 1), (True, 0.2, 32, 1)])
def test_edges(dropout_exit, p, out_dim, B):
    """No site and p = 0: every sample is the same, so the raw sums obey S2 * T == S1^2 exactly at T = 8 (sums of 8 equal fp32 values
    and of their squares are exact in float64, in any order) and the variance is exactly 0.  Two classes: lanes 2 .. 63 carry nothing;
    32 classes: the widest classifier."""
    _, x, eng, logits, r = run(mirror(dropout_exit, p, out_dim), synthetic_images(B, 1234, channels=1, size=28), 8)
    assert_close(logits, r, reference(dropout_exit, p, B, out_dim, 8))
    if not dropout_exit or p == 0.0:
        S = eng.accumulate(x, eng.new_moments(B), 0, 8, SEED)
        assert np.array_equal(logits, np.broadcast_to(logits[:1], logits.shape))
        assert torch.equal(S[1] * 8, S[0] * S[0]) and np.all(r["var"] == 0)


def test_branch_geometry():
    """ex1conv1 with a value of its own in every tap, one bright pixel per image around the corners of the four 5x5 windows: stride 7
    without padding reads rows and columns 0..4 and 7..11 of the pooled map (image rows 0..9 and 14..23)."""
    m = mirror(False)
    with torch.no_grad():
        m.ex1conv1.weight.copy_(((torch.arange(25.).view(1, 1, 5, 5) + 1) / 250) * torch.linspace(-1, 1, 400).view(20, 20, 1, 1))
    pixels = torch.tensor([(0, 0), (9, 9), (10, 4), (13, 13), (14, 14), (9, 23), (24, 15), (23, 23), (27, 27)])
    x = torch.zeros(len(pixels), 1, 28, 28)
    x[torch.arange(len(pixels)), 0, pixels[:, 0], pixels[:, 1]] = 4.0
    _, _, _, logits, r = run(m, x, 1)
    assert_close(logits, r, forward64(m.cpu(), x, 1))
