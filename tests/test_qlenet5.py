"""The quantised LeNet-5 on the device (csrc/qlenet5.hip behind ``engine.LeNet5Engine``, ``LeNet5MC(quant_tbit=W, quant_ibit=I)``) against a
plain integer forward of the contract in include/bayesnn_fpga_amd.h: float64 convolutions of integer-valued tensors (exact), the keep masks
of ``oracle.philox``, the two rounded steps of every layer in ``np.float32``.  The weights are drawn as integer codes and set as
code * 2^-F, so weight quantisation is the identity.  Logits: tolerance ZERO (every sum is an exact integer below 2^24 and the float steps are
the contract's own); mean and variance: the project's 1e-3 against the float64 softmax of the reference logits (tests/test_lenet5.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.synthetic import synthetic_images
from oracle import philox

gpu = pytest.mark.gpu
SEED = 77
LAYERS = ("conv1", "conv2", "fc1", "fc2")
# standard deviation of the drawn weight VALUES and the bias VALUE per layer: small enough that the codes of every layer neither all vanish nor
# all saturate behind the 2x2 / 7x7 maxima (test_reference_inputs_exercise_the_arithmetic holds the draw to that)
DRAW = {(6, 0): ((0.12, 0.035, 0.10, 0.6), (-0.1, -0.45, -0.1, 0.0)), (8, 0): ((0.12, 0.035, 0.10, 0.5), (0.0, -0.4, -0.1, 0.0)),
        (8, 3): ((0.12, 0.04, 0.12, 0.5), (0.0, -0.45, -0.1, 0.0)), (2, 0): ((0.27, 0.2, 0.3, 0.5), (0.0, -0.5, 0.0, 0.0))}


@functools.lru_cache(maxsize=None)
def codes(W, I, out_dim=10):
    """Seeded integer codes {name: int64 array} of the eight parameters."""
    rng, fbits, out = np.random.default_rng(1000 * W + I), W - 1 - I, {}
    shapes = dict(conv1=(20, 1, 5, 5), conv2=(20, 20, 5, 5), fc1=(100, 80), fc2=(out_dim, 100))
    for name, sd, mu in zip(LAYERS, *DRAW[W, I]):
        for part, v in ((".weight", rng.normal(0.0, sd, shapes[name])), (".bias", rng.normal(mu, sd, shapes[name][0]))):
            out[name + part] = np.clip(np.rint(v * 2.0 ** fbits), -2 ** (W - 1), 2 ** (W - 1) - 1).astype(np.int64)
    return out


def mirror(W, I, k, p, out_dim=10):
    m = bx.LeNet5MC(num_bayes_layer=k, dropout_p=p, out_dim=out_dim, quant_tbit=W, quant_ibit=I)
    m.load_state_dict({n: torch.from_numpy(v * 2.0 ** -(W - 1 - I)).float() for n, v in codes(W, I, out_dim).items()})
    return m


@functools.lru_cache(maxsize=None)
def reference(W, I, k, p, B, n, out_dim=10):
    """fp32 logits [n, 1, B, C], float64 mean and variance [1, B, C], and the activation codes of sample 0 per layer."""
    q = {name: torch.from_numpy(v).double() for name, v in codes(W, I, out_dim).items()}
    fbits, amax = W - 1 - I, 2 ** W - 1
    on = [loc >= 3 - k for loc in range(3)]
    ids = np.cumsum(on) - 1
    ties = []

    def rne(v):                      # v: float64, exact; counts the exact ties it rounds
        ties.append(int((np.abs(v - np.floor(v) - 0.5) == 0).sum()))
        return np.rint(v)

    def keep(v, loc, t):             # the kept codes and the layer's d
        if not on[loc]:
            return v, np.float32(1.0)
        return v * torch.from_numpy(philox.elementwise_mask(v.shape, SEED, int(ids[loc]), t, p)).double(), philox.drop_scale(p)

    def affine(acc, d, bias):        # acc: exact integers in float64 -> y in fp32, two rounded steps
        y = (acc.numpy().astype(np.float32) * np.float32(2.0 ** -(W + fbits))) * np.float32(d)
        return y + (bias.numpy() * 2.0 ** -fbits).astype(np.float32).reshape((1, -1) + (1,) * (acc.dim() - 2))

    act = lambda y: torch.from_numpy(np.clip(rne(y.astype(np.float64) * 2.0 ** W), 0, amax))
    x8 = torch.from_numpy(np.clip(np.rint(synthetic_images(B, 1234, channels=1, size=28).double().numpy() * 256.0), 0, 255))
    pre = F.conv2d(x8, q["conv1.weight"], q["conv1.bias"] * 256.0, padding=2).numpy()
    p1 = F.max_pool2d(torch.from_numpy(np.clip(rne(pre / 2.0 ** (7 - I)), 0, amax)), 2)
    logits, layers = [], None
    for t in range(n):
        a, d = keep(p1, 0, t)
        f = F.max_pool2d(act(affine(F.conv2d(a, q["conv2.weight"], padding=2), d, q["conv2.bias"])), 7).flatten(1)
        a, d = keep(f, 1, t)
        h = act(affine(F.linear(a, q["fc1.weight"]), d, q["fc1.bias"]))
        a, d = keep(h, 2, t)
        logits.append(affine(F.linear(a, q["fc2.weight"]), d, q["fc2.bias"]))
        layers = layers or dict(p1=p1.numpy(), feat=f.numpy(), hidden=h.numpy(), ties=sum(ties))
    logits = np.stack(logits)[:, None]
    probs = torch.softmax(torch.from_numpy(logits).double(), -1)
    return logits, probs.mean(0).numpy(), probs.var(0, unbiased=False).numpy(), layers


# (W, I) x k x p x (B, T), pruned: every (W, I) meets every k, both keep formats (p = 0.25: 2 bits, 0.2: 16 bits) and the three launch forms
# (B = 1, 7: every sample a workgroup of its own, joined; B = 260: one chunk of four samples inside the kernel's loop)
CASES = [(W, I, k, (0.25, 0.2)[(k + i + j) % 2], *((1, 10), (7, 10), (260, 4))[(k + i + j) % 3], 10)
         for i, (W, I) in enumerate(((6, 0), (8, 0), (8, 3), (2, 0))) for k in range(4) for j in range(2 if k else 1)]
CASES.append((8, 0, 3, 0.2, 7, 10, 3))


@gpu
@pytest.mark.parametrize("W,I,k,p,B,n,out_dim", CASES)
def test_logits_bit_for_bit_and_moments(W, I, k, p, B, n, out_dim):
    m = mirror(W, I, k, p, out_dim).to("cuda:0").eval()
    x = synthetic_images(B, 1234, channels=1, size=28).to("cuda:0")
    eng = m.engine(x.device, max_batch=B)
    logits, mean, var, _ = reference(W, I, k, p, B, n, out_dim)
    got = eng.forward_samples(x, n, seed=SEED).cpu().numpy()
    print(f"logits: {int((got != logits).sum())} of {logits.size} differ, max |error| {np.abs(got - logits).max():.3e}")
    assert np.array_equal(got, logits)
    r = eng.predict(x, n, seed=SEED)
    for name, ref in (("mean", mean), ("var", var)):
        print(f"{name}: max |error| {np.abs(r[name].cpu().numpy() - ref).max():.3e} (tolerance 1.0e-03)")
        np.testing.assert_allclose(r[name].cpu().numpy(), ref, rtol=0, atol=1e-3, err_msg=name)


@gpu
def test_sample_addressing():
    m = mirror(6, 0, 3, 0.2).to("cuda:0").eval()
    x = synthetic_images(7, 1234, channels=1, size=28).to("cuda:0")
    eng = m.engine(x.device, max_batch=7)
    logits = eng.forward_samples(x, 10, seed=SEED).cpu().numpy()
    assert np.array_equal(eng.forward_samples(x, 4, seed=SEED, t_begin=6).cpu().numpy(), logits[6:])
    m.mc_seed = SEED
    passes = np.stack([m(x)[0].cpu().numpy() for _ in range(10)])
    assert np.array_equal(passes, logits[:, 0]) and m.mc_pass == 10


@pytest.mark.parametrize("W,I", sorted(DRAW))
def test_reference_inputs_exercise_the_arithmetic(W, I):
    """On the reference alone (no GPU): at every layer at least a tenth of the activation codes are nonzero and at least a tenth are below
    saturation, some rne meets an exact tie, and at W = 8 the pooled conv1 map holds a code >= 128 (the signed-operand path) and some layer
    clips at 255."""
    amax = 2 ** W - 1
    layers = reference(W, I, 3, 0.25, 7, 10)[3]
    for name in ("p1", "feat", "hidden"):
        v = layers[name]
        print(f"W={W} I={I} {name}: nonzero {np.mean(v > 0):.3f}, below saturation {np.mean(v < amax):.3f}, max {v.max():.0f}")
        assert np.mean(v > 0) >= 0.1 and np.mean(v < amax) >= 0.1, name
    assert layers["ties"] > 0
    if W == 8:
        assert layers["p1"].max() >= 128 and max(layers[name].max() for name in ("p1", "feat", "hidden")) == 255
