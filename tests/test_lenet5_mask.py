"""Masksembles LeNet-5 on the device (csrc/lenet5_mask.hip behind ``engine.LeNet5Engine``) against a plain float64 torch forward of its six
layers with ``x * masks[t % M]`` over the channel axis, and bit for bit against ``lenet5_kernel`` on weights zeroed where a mask drops.
The masks are seeded Bernoulli(0.5) rows, not ``generation_wrapper``'s: the kernel may assume no structure.  Tolerances are the project's
(tests/test_lenet5.py): 5e-3 * max(1, max|logit|) on logits, 1e-3 on mean and variance; the arithmetic is that kernel's minus the rescale,
whose CPU emulation (P1 and conv2's operands in fp16, fp32 accumulation) stays below 8.9e-3 on logits of magnitude 22-40, 2.3e-4 on the
mean and 1.8e-4 on the variance on these inputs and weights."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from tests.helpers import build_seeded

pytestmark = pytest.mark.gpu
images = lambda B: synthetic_images(B, 1234, channels=1, size=28)


def mirror(k, M, zero_row=None):
    m = synthetic_weights_(build_seeded(bx.LeNet5MC, dict(num_bayes_layer=k, mask_type="mask", num_masks=M)), 0)
    rng = np.random.default_rng(100 * k + M)
    for layer in m.mask_layers():
        layer.masks.data = torch.from_numpy((rng.random(tuple(layer.masks.shape)) < 0.5).astype(np.float32))
    if zero_row is not None:
        m.drop.masks.data[zero_row] = 0
    return m


@functools.lru_cache(maxsize=None)
def reference(k, M, B, T, t_begin):
    """float64 logits [T, 1, B, C], mean and variance [1, B, C] of the samples t_begin .. t_begin + T - 1."""
    m = mirror(k, M)
    w = {n: v.double() for n, v in m.state_dict().items()}
    site = lambda v, name, t: v * w[name + ".masks"][t % M].view(1, -1, *[1] * (v.dim() - 2)) if hasattr(m, name) else v
    p1 = F.max_pool2d(F.relu(F.conv2d(images(B).double(), w["conv1.weight"], w["conv1.bias"], padding=2)), 2)
    logits = []
    for t in range(t_begin, t_begin + T):
        f = F.max_pool2d(F.relu(F.conv2d(site(p1, "drop_a", t), w["conv2.weight"], w["conv2.bias"], padding=2)), 7).flatten(1)
        h = F.relu(F.linear(site(f, "drop_b", t), w["fc1.weight"], w["fc1.bias"]))
        logits.append(F.linear(site(h, "drop", t), w["fc2.weight"], w["fc2.bias"]))
    logits = torch.stack(logits)[:, None]
    probs = torch.softmax(logits, -1)
    return logits.numpy(), probs.mean(0).numpy(), probs.var(0, unbiased=False).numpy()


def engine(m, B):
    m = m.to("cuda:0").eval()
    x = images(B).to("cuda:0")
    return m, x, m.engine(x.device, max_batch=B)


# B = 1 and 7: one pass per workgroup plus the join; T = 2M + 1: unequal multiplicities and a wrapped mask index; B = 260: one chunk that
# loops over the M passes inside the kernel
@pytest.mark.parametrize("shape", [(1, 0, 0), (7, 1, 2), (260, 0, 0)], ids=["B1", "B7", "B260"])
@pytest.mark.parametrize("M", [3, 4])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_parity_with_the_float64_reference(k, M, shape):
    B, T, t_begin = shape[0], (2 * M + 1 if shape[1] else M), shape[2]
    _, x, eng = engine(mirror(k, M), B)
    logits = eng.forward_samples(x, T, t_begin=t_begin).cpu().numpy()
    r = {n: v.cpu().numpy() for n, v in eng.predict(x, T, t_begin=t_begin).items()}
    want = reference(k, M, B, T, t_begin)
    for name, got, ref, tol in (("logits", logits, want[0], 5e-3 * max(1.0, float(np.abs(want[0]).max()))), ("mean", r["mean"], want[1], 1e-3),
                                ("var", r["var"], want[2], 1e-3)):
        print(f"{name}: max |error| {np.abs(got - ref).max():.3e} (tolerance {tol:.1e})")
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol, err_msg=name)


@pytest.mark.parametrize("B", [7, 260])
def test_bit_for_bit_against_lenet5_kernel_on_zeroed_weights(B):
    """Row m of the Masksembles engine = the deterministic model whose conv2 / fc1 / fc2 weights are zero where mask m drops their input:
    pins the operand masking and the arithmetic order.  Mask row 1 of site C is all zero: exactly the fc2 bias."""
    M = 4
    masked, x, eng = engine(mirror(3, M, zero_row=1), B)
    rows = eng.forward_samples(x, M).cpu().numpy()
    for m in range(M):
        plain = synthetic_weights_(build_seeded(bx.LeNet5MC, dict(num_bayes_layer=0)), 0)
        with torch.no_grad():
            plain.conv2.weight *= masked.drop_a.masks[m].cpu().view(1, 20, 1, 1)
            plain.fc1.weight *= masked.drop_b.masks[m].cpu().view(1, 80)
            plain.fc2.weight *= masked.drop.masks[m].cpu().view(1, 100)
        _, _, ref = engine(plain, B)
        assert np.array_equal(ref.forward_samples(x, 1).cpu().numpy()[0], rows[m]), m
    assert np.array_equal(rows[1, 0], np.broadcast_to(masked.fc2.bias.detach().cpu().numpy(), rows[1, 0].shape))


def test_repeats_and_addressing():
    M, B = 4, 7
    T = 2 * M + 1
    m, x, eng = engine(mirror(3, M), B)
    rows = eng.forward_samples(x, T).cpu().numpy()
    for t in range(T - M):
        assert np.array_equal(rows[t], rows[t + M]), t
    for t in range(M):
        assert np.array_equal(eng.forward_samples(x, 1, t_begin=t).cpu().numpy()[0], rows[t]), t
    one = eng.predict(x, T)
    S = eng.new_moments(B)
    eng.accumulate(x, S, 0, 4)
    eng.accumulate(x, S, 4, T - 4)
    two = eng.finalize(S, T)
    for name in ("mean", "var"):          # the float64 sums only change their order
        np.testing.assert_allclose(two[name].cpu().numpy(), one[name].cpu().numpy(), rtol=0, atol=1e-12)
    passes, cnts = zip(*[(m(x)[0].cpu().numpy(), [layer.cnt for layer in m.mask_layers()]) for _ in range(M)])
    assert np.array_equal(np.stack(passes), rows[:M, 0]) and m.mc_pass == M and list(cnts) == [[(t + 1) % M] * 3 for t in range(M)]
    m.mc_pass = 0
    for layer in m.mask_layers():         # a stream that starts at counter 3: its rows are the rows from 3 on
        layer.cnt = 3
    assert np.array_equal(np.stack([m(x)[0].cpu().numpy() for _ in range(3)]), rows[3:6, 0])
    assert np.array_equal(eng.forward_samples(x, 3, cnt0=3).cpu().numpy(), rows[3:6])
