"""The quantised multi-exit LeNet-5 on the device (csrc/qlenet5_me.hip behind ``engine.LeNet5Engine``, ``LeNet5MCEarlyExit(quant_tbit=W,
quant_ibit=I)``) against a plain integer forward of the contract in include/bayesnn_fpga_amd.h, in the manner of tests/test_qlenet5.py:
float64 convolutions of integer-valued tensors (exact), the keep masks of ``oracle.philox``, the two rounded steps of every layer in
``np.float32``.  The weights are drawn as integer codes and set as code * 2^-F, so weight quantisation is the identity.  Logits: tolerance
ZERO; mean and variance: the project's 1e-3 against the float64 softmax of the reference logits."""
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
LAYERS = ("conv1", "conv2", "fc1", "ex1conv1", "ex1fc1", "fc2", "ex1linear")      # (the two classifiers last: everything else is the same for every out_dim)
# standard deviation of the drawn weight VALUES and the mean of the bias VALUES per layer (the trunk's are those of tests/test_qlenet5.py
# with conv2's bias moved: no dropout scale in front of conv2 here): chosen on the reference alone so that
# test_reference_inputs_exercise_the_arithmetic holds
DRAW = {(6, 0): ((0.12, 0.035, 0.10, 0.035, 0.10, 0.6, 0.6), (-0.1, -0.3, -0.1, -0.1, -0.1, 0.0, 0.0)),
        (8, 0): ((0.12, 0.035, 0.10, 0.035, 0.10, 0.5, 0.5), (0.0, -0.4, -0.1, -0.1, -0.1, 0.0, 0.0)),
        (8, 3): ((0.12, 0.04, 0.12, 0.04, 0.12, 0.5, 0.5), (0.0, -0.45, -0.1, -0.1, -0.1, 0.0, 0.0)),
        (2, 0): ((0.27, 0.2, 0.3, 0.2, 0.3, 0.5, 0.5), (0.0, -0.7, 0.0, -0.25, 0.0, 0.0, 0.0))}


@functools.lru_cache(maxsize=None)
def codes(W, I, out_dim=10):
    """Seeded integer codes {name: int64 array} of the fourteen parameters."""
    rng, fbits, out = np.random.default_rng(2000 * W + I), W - 1 - I, {}
    shapes = dict(conv1=(20, 1, 5, 5), conv2=(20, 20, 5, 5), fc1=(100, 80), fc2=(out_dim, 100), ex1conv1=(20, 20, 5, 5), ex1fc1=(100, 80),
                  ex1linear=(out_dim, 100))
    for name, sd, mu in zip(LAYERS, *DRAW[W, I]):
        for part, v in ((".weight", rng.normal(0.0, sd, shapes[name])), (".bias", rng.normal(mu, sd, shapes[name][0]))):
            out[name + part] = np.clip(np.rint(v * 2.0 ** fbits), -2 ** (W - 1), 2 ** (W - 1) - 1).astype(np.int64)
    return out


def mirror(W, I, dropout_exit, p, out_dim=10):
    m = bx.LeNet5MCEarlyExit(dropout_exit=dropout_exit, dropout_p=p, out_dim=out_dim, quant_tbit=W, quant_ibit=I)
    m.load_state_dict({n: torch.from_numpy(v * 2.0 ** -(W - 1 - I)).float() for n, v in codes(W, I, out_dim).items()})
    return m


@functools.lru_cache(maxsize=None)
def reference(W, I, dropout_exit, p, B, n, out_dim=10):
    """fp32 logits [n, 2, B, C] (early exit, main exit), float64 mean and variance [2, B, C], and the activation codes per layer."""
    q = {name: torch.from_numpy(v).double() for name, v in codes(W, I, out_dim).items()}
    fbits, amax = W - 1 - I, 2 ** W - 1
    ties = []

    def rne(v):                      # v: float64, exact; counts the exact ties it rounds
        ties.append(int((np.abs(v - np.floor(v) - 0.5) == 0).sum()))
        return np.rint(v)

    def affine(acc, d, bias):        # acc: exact integers in float64 -> y in fp32, two rounded steps
        y = (acc.numpy().astype(np.float32) * np.float32(2.0 ** -(W + fbits))) * np.float32(d)
        return y + (bias.numpy() * 2.0 ** -fbits).astype(np.float32).reshape((1, -1) + (1,) * (acc.dim() - 2))

    act = lambda y: torch.from_numpy(np.clip(rne(y.astype(np.float64) * 2.0 ** W), 0, amax))
    layer = lambda a, name, **kw: affine((F.conv2d if a.dim() == 4 else F.linear)(a, q[name + ".weight"], **kw), 1.0, q[name + ".bias"])
    x8 = torch.from_numpy(np.clip(np.rint(synthetic_images(B, 1234, channels=1, size=28).double().numpy() * 256.0), 0, 255))
    pre = F.conv2d(x8, q["conv1.weight"], q["conv1.bias"] * 256.0, padding=2).numpy()
    p1 = F.max_pool2d(torch.from_numpy(np.clip(rne(pre / 2.0 ** (7 - I)), 0, amax)), 2)
    feat = F.max_pool2d(act(layer(p1, "conv2", padding=2)), 7).flatten(1)
    hidden = act(layer(feat, "fc1"))
    efeat = act(layer(p1, "ex1conv1", stride=7)).flatten(1)
    ehidden = act(layer(efeat, "ex1fc1"))
    layers = dict(p1=p1.numpy(), feat=feat.numpy(), hidden=hidden.numpy(), efeat=efeat.numpy(), ehidden=ehidden.numpy(), ties=sum(ties))
    d = philox.drop_scale(p) if dropout_exit else np.float32(1.0)
    logits = []
    for t in range(n):
        row = []
        for site, (h, name) in enumerate(((ehidden, "ex1linear"), (hidden, "fc2"))):
            a = h * torch.from_numpy(philox.elementwise_mask((B, 100), SEED, site, t, p)).double() if dropout_exit else h
            row.append(affine(F.linear(a, q[name + ".weight"]), d, q[name + ".bias"]))
        logits.append(np.stack(row))
    logits = np.stack(logits)
    probs = torch.softmax(torch.from_numpy(logits).double(), -1)
    return logits, probs.mean(0).numpy(), probs.var(0, unbiased=False).numpy(), layers


# (W, I, dropout_exit, p, B, T, out_dim), pruned: every (W, I) meets the unmasked loop and both keep formats (p = 0.25: 2 bits, 0.2: 16 bits);
# B = 7 holds images whose first keep byte starts four elements early; T = 1: the odd-parity waves have no sample, 5: uneven shares;
# out_dim 3 and 32: the lane bounds of the classifier and of the softmax shuffles
CASES = [(6, 0, True, 0.25, 1, 1, 10), (6, 0, True, 0.2, 7, 5, 10), (6, 0, False, 0.2, 7, 10, 10),
         (8, 0, True, 0.2, 7, 10, 10), (8, 0, True, 0.25, 1, 5, 3), (8, 0, False, 0.25, 1, 1, 32),
         (8, 3, True, 0.25, 7, 10, 32), (8, 3, True, 0.2, 1, 1, 10), (8, 3, False, 0.2, 7, 5, 3),
         (2, 0, True, 0.2, 7, 10, 3), (2, 0, True, 0.25, 7, 5, 32), (2, 0, False, 0.25, 1, 10, 10)]


@gpu
@pytest.mark.parametrize("W,I,dropout_exit,p,B,n,out_dim", CASES)
def test_logits_bit_for_bit_and_moments(W, I, dropout_exit, p, B, n, out_dim):
    m = mirror(W, I, dropout_exit, p, out_dim).to("cuda:0").eval()
    x = synthetic_images(B, 1234, channels=1, size=28).to("cuda:0")
    eng = m.engine(x.device, max_batch=B)
    logits, mean, var, _ = reference(W, I, dropout_exit, p, B, n, out_dim)
    got = eng.forward_samples(x, n, seed=SEED).cpu().numpy()
    assert eng.dtype == "i8" and got.shape == (n, 2, B, out_dim)
    for e in range(2):
        print(f"exit {e} logits: {int((got[:, e] != logits[:, e]).sum())} of {logits[:, e].size} differ, max |error| {np.abs(got[:, e] - logits[:, e]).max():.3e}")
    assert np.array_equal(got, logits)
    r = eng.predict(x, n, seed=SEED)
    for name, ref in (("mean", mean), ("var", var)):
        print(f"{name}: max |error| {np.abs(r[name].cpu().numpy() - ref).max():.3e} (tolerance 1.0e-03)")
        np.testing.assert_allclose(r[name].cpu().numpy(), ref, rtol=0, atol=1e-3, err_msg=name)


@gpu
def test_sample_addressing():
    """The parity of a sample is counted from the call's first sample, its logits depend on t alone."""
    m = mirror(6, 0, True, 0.2).to("cuda:0").eval()
    x = synthetic_images(7, 1234, channels=1, size=28).to("cuda:0")
    eng = m.engine(x.device, max_batch=7)
    logits = eng.forward_samples(x, 10, seed=SEED).cpu().numpy()
    assert np.array_equal(logits, reference(6, 0, True, 0.2, 7, 10)[0])
    assert np.array_equal(eng.forward_samples(x, 4, seed=SEED, t_begin=6).cpu().numpy(), logits[6:])
    m.mc_seed = SEED
    passes = np.stack([np.stack([o.cpu().numpy() for o in m(x)]) for _ in range(10)])
    assert np.array_equal(passes, logits) and m.mc_pass == 10
    with pytest.raises(ValueError, match="fp16 model only"):
        eng.predict_early_exit(x, 4, 0.9)


@pytest.mark.parametrize("W,I", sorted(DRAW))
def test_reference_inputs_exercise_the_arithmetic(W, I):
    """On the reference alone (no GPU): at every layer of both branches at least a tenth of the activation codes are nonzero and at least a
    tenth are below saturation, some rne meets an exact tie, and at W = 8 the pooled conv1 map holds a code >= 128 (the signed-operand path)
    and some layer clips at 255."""
    amax = 2 ** W - 1
    layers = reference(W, I, True, 0.25, 7, 10)[3]
    names = ("p1", "feat", "hidden", "efeat", "ehidden")
    for name in names:
        v = layers[name]
        print(f"W={W} I={I} {name}: nonzero {np.mean(v > 0):.3f}, below saturation {np.mean(v < amax):.3f}, max {v.max():.0f}")
        assert np.mean(v > 0) >= 0.1 and np.mean(v < amax) >= 0.1, name
    assert layers["ties"] > 0
    if W == 8:
        assert layers["p1"].max() >= 128 and max(layers[name].max() for name in names) == 255
