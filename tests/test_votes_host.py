"""Vote counts without a GPU: the ctypes bindings and the C ABI's host-side validation (no call reaches a kernel), the numpy restatements
``vote_counts_numpy`` / ``vote_readout_numpy`` against an independent torch formulation (softmax, cumsum over the exits, arg-max, bincount),
the tie rule, the non-finite rule, the read-out identities, and the consistency of the maps (a diagonal matrix is a vector scaling, one-hot
weight rows are that exit's own classifier)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.uncertainty import calibrated_logits, vote_counts_numpy, vote_readout_numpy, weighted_exit_ensembles
from tests.helpers import build_seeded
from tests.test_pass_accuracy_host import make_case

NEW = ("bmi_forward_mcd_votes", "bmi_vote_counts", "bmi_finalize_votes")
# (T, E, B, C, scale, seed) of make_case: the issue's cases, shared with tests/test_votes.py — C of 2, 7, 64, 65 and 128 (both lane halves
# and the boundary), E of 1 and 32, a batch that does not fill a block, the reference's batch of 250
CASES = [(3, 4, 37, 10, 3, 0), (2, 5, 19, 100, 4, 1), (2, 1, 8, 7, 2, 2), (2, 3, 70, 128, 5, 3), (1, 2, 5, 2, 1, 4), (2, 32, 3, 65, 3, 6),
         (5, 4, 9, 64, 3, 7), (4, 4, 250, 100, 3, 5)]
MAPS = ("none", "tau", "vector", "matrix")
GAP = 1e-6                    # the margin of tests/test_pass_accuracy.py: five orders above what an exp and its summation tree can move
case_id = lambda c: "T{}E{}B{}C{}".format(*c[:4])


def make_map(kind, E, C_, seed):
    """The issue's maps as keyword arguments of ``vote_counts_numpy``: tau in U(0.5, 3); vector a in U(0.5, 2), b = 0.5 N; matrix = a
    diagonal like a plus 0.05 N off the diagonal, with a bias like b"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "none":
        return {}
    if kind == "tau":
        return dict(tau=rng.uniform(0.5, 3.0, E))
    a = rng.uniform(0.5, 2.0, (E, C_)).astype(np.float32)
    b = (0.5 * rng.standard_normal((E, C_))).astype(np.float32)
    if kind == "vector":
        return dict(scale=a, bias=b)
    M = (0.05 * rng.standard_normal((E, C_, C_))).astype(np.float32)
    M[:, np.arange(C_), np.arange(C_)] = a
    return dict(matrix=M, bias=b)


def make_weights(E, seed):
    """Lower-triangular float64 [E, E], positive entries, every row summing to 1"""
    rng = np.random.default_rng(2000 + seed)
    W = np.tril(rng.uniform(0.2, 1.0, (E, E)))
    return W / W.sum(axis=1, keepdims=True)


def vote_gap(l, weights=None, **cal):
    """The tie-freeness of an input: (no row of z has two equal top entries, the least relative gap between the top two entries of any
    ensemble row q) — float64 on the host, the definition's own z and q"""
    z32, W = calibrated_logits(l, weights=weights, **cal)
    top = np.sort(z32, axis=-1)
    no_equal = bool((top[..., -1] != top[..., -2]).all())
    z = z32.astype(np.float64)
    ex = np.exp(z - z.max(-1, keepdims=True))
    p = ex / ex.sum(-1, keepdims=True)
    if W is None:
        q = np.cumsum(p, axis=1) / np.arange(1, p.shape[1] + 1)[None, :, None, None]
    else:
        q = np.stack([weighted_exit_ensembles(p[t], W) for t in range(p.shape[0])])
    qs = np.sort(q, axis=-1)
    return no_equal, float(((qs[..., -1] - qs[..., -2]) / qs[..., -1]).min())


def torch_votes(l, weights=None, **cal):
    """V [2, E, B, C] through F.softmax, cumsum (or a matmul with the weights) over the exits, argmax and bincount"""
    z32, W = calibrated_logits(l, weights=weights, **cal)
    T, E, B, C_ = z32.shape
    zt = torch.from_numpy(z32)
    p = F.softmax(zt.double(), dim=-1)
    if W is None:
        q = torch.cumsum(p, dim=1) / torch.arange(1, E + 1, dtype=torch.float64)[None, :, None, None]
    else:
        q = torch.einsum("ei,tibc->tebc", torch.from_numpy(W), p)
    out = np.zeros((2, E, B, C_), dtype=np.int32)
    for kind, score in enumerate((zt, q)):
        k = score.argmax(dim=-1)                                      # [T, E, B]
        for e in range(E):
            for b in range(B):
                out[kind, e, b] = torch.bincount(k[:, e, b], minlength=C_).numpy()
    return out


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600


def test_c_abi_validation():
    """Null pointers, counts below 1, two maps at once, a bias without its map, a bad tau, the shape limits: decided on the host, before any
    launch (the device pointers are never dereferenced)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID, UNSUPPORTED = -22, -95
    T, E, B, Cd = 3, 4, 7, 10
    tau = (C.c_float * 33)(*([1.5] * 33))
    # bmi_vote_counts(logits, T, E, B, C, tau, scale, bias, matrix, W, V, nonfinite, stream)
    ok = [fake, T, E, B, Cd, None, None, None, None, None, fake, None, None]
    for i in (0, 10):
        args = list(ok)
        args[i] = None
        assert lib.bmi_vote_counts(*args) == INVALID, i
    for i in (1, 2, 3, 4):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_vote_counts(*args) == INVALID, (i, v)
    for maps in (dict(tau=tau, scale=fake, bias=fake), dict(tau=tau, matrix=fake, bias=fake), dict(scale=fake, matrix=fake, bias=fake),
                 dict(bias=fake), dict(scale=fake), dict(matrix=fake), dict(tau=tau, bias=fake)):
        args = list(ok)
        args[5], args[6], args[7], args[8] = maps.get("tau"), maps.get("scale"), maps.get("bias"), maps.get("matrix")
        assert lib.bmi_vote_counts(*args) == INVALID, sorted(maps)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        args = list(ok)
        args[5] = (C.c_float * E)(1.0, bad, 1.0, 1.0)
        assert lib.bmi_vote_counts(*args) == INVALID, bad
    args = list(ok)
    args[4] = 129
    assert lib.bmi_vote_counts(*args) == UNSUPPORTED
    args = list(ok)
    args[2], args[5] = 33, tau
    assert lib.bmi_vote_counts(*args) == UNSUPPORTED
    args = list(ok)
    args[1], args[3] = 1 << 15, 1 << 10                              # T * B = 2^25: the launch grid
    assert lib.bmi_vote_counts(*args) == UNSUPPORTED
    # bmi_finalize_votes(n_exits, batch, out_dim, V, vote_class, variation_ratio, vote_entropy, stream)
    ok = [E, B, Cd, fake, fake, fake, fake, None]
    for i in (3, 4, 5, 6):
        args = list(ok)
        args[i] = None
        assert lib.bmi_finalize_votes(*args) == INVALID, i
    for i in (0, 1, 2):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_finalize_votes(*args) == INVALID, (i, v)
    args = list(ok)
    args[0], args[1] = 1 << 12, 1 << 12                              # 2 * E * B = 2^25
    assert lib.bmi_finalize_votes(*args) == UNSUPPORTED
    # bmi_forward_mcd_votes: a null handle, before anything else
    assert lib.bmi_forward_mcd_votes(None, fake, 1, 0, 0, 1, 0, 0, *([fake] * 8), None, fake, 1 << 20, fake, 1 << 20, None) == INVALID


def test_forward_entry_point_checks_arguments_before_any_launch():
    """bmi_forward_mcd_votes on a graph that lives on the CPU (a call that got as far as a launch would fail with a HIP error instead):
    bmi_forward_mcd_ensemble's answers, a null V, an undersized scratch; nothing is written."""
    kw = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
    cg = CompiledGraph(build_seeded(ResNet18MCEarlyExit, kw), "cpu", 8, 4, dtype="f16")
    lib, h, ws_ok, E = _lib.lib(), cg.handle, cg.workspace_bytes, cg.n_exits
    need = lib.bmi_ensemble_scratch_bytes(h, 8)
    assert need == 4 * E * 8 * 10 * 4
    buf = np.zeros(64, dtype=np.float64)                  # a non-null address; no row gets far enough to use it
    p = buf.ctypes.data

    def fv(h=h, x=p, batch=8, t_begin=0, t_count=4, S1=p, SH=p, Q1=p, QH=p, V=p, nf=p, scratch=p, sbytes=need, nbytes=ws_ok):
        return lib.bmi_forward_mcd_votes(h, x, batch, 0, t_begin, t_count, 7, 0, S1, p, p, SH, Q1, p, QH, V, nf, scratch, sbytes, p, nbytes, None)

    rows = [
        (fv(h=None), -22), (fv(SH=None), -22), (fv(V=None), -22), (fv(Q1=None), -22), (fv(QH=None), -22), (fv(scratch=None), -22),
        (fv(batch=0), -22), (fv(batch=9), -22), (fv(sbytes=need - 1), -12), (fv(sbytes=0), -12), (fv(sbytes=need - 1, nbytes=ws_ok - 1), -12),
        (fv(x=None), -22), (fv(S1=None), -22), (fv(t_count=0), -22), (fv(t_begin=-1), -22), (fv(nbytes=ws_ok - 1), -12),
        (fv(nf=None, nbytes=ws_ok - 1), -12),                # the counter stays optional
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]
    assert not buf.any()


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_numpy_restatement_against_torch_on_gap_checked_input(case, kind, weighted):
    l, _ = make_case(*case)
    T, E, B, C_ = l.shape
    cal = make_map(kind, E, C_, case[5])
    W = make_weights(E, case[5]) if weighted else None
    no_equal, gap = vote_gap(l, weights=W, **cal)
    print(f"{case} {kind} weighted={weighted}: least relative top-2 gap of q {gap:.2e}")
    assert no_equal and gap >= GAP                 # (a condition on the input, not a measurement of the code)
    V, nf = vote_counts_numpy(l, weights=W, **cal)
    assert V.shape == (2, E, B, C_) and V.dtype == np.int32 and nf == 0
    assert (V.sum(-1) == T).all()                  # every pass votes once per (kind, exit, image)
    assert np.array_equal(V, torch_votes(l, weights=W, **cal))
    if not weighted:
        assert np.array_equal(V[1, 0], V[0, 0])    # the ensemble of exit 0 alone is exit 0
    if T > 1 and B * E > 8:
        assert (V.max(-1) < T).any()               # the passes disagree somewhere: a kernel that counts one pass T times fails


def test_constructed_ties_take_the_lower_index():
    # two equal top logits: the lower index
    l = np.zeros((1, 1, 3, 5), np.float32)
    l[0, 0, 0, [1, 3]] = 2.0
    l[0, 0, 1, [4, 0]] = 1.0
    l[0, 0, 2, :] = -3.0                           # a whole row tied
    V, nf = vote_counts_numpy(l)
    assert nf == 0 and V[0, 0].argmax(-1).tolist() == [1, 0, 0] and (V.sum(-1) == 1).all()
    assert np.array_equal(V[1], V[0])              # equal logits give bit-equal exponentials: exit 0's ensemble ties where its logits do
    # equal q from mirrored exits: exit 1 is exit 0 with classes 0 and 1 swapped — neighbours, so that every summation tree adds the same
    # pairs and the two rows' exponential sums are the same bits — and q_1 ties at classes 0 and 1 exactly (a + b == b + a)
    l = np.zeros((2, 2, 1, 4), np.float32)
    l[:, 0, 0] = [3.0, 1.0, 0.0, -1.0]
    l[:, 1, 0] = [1.0, 3.0, 0.0, -1.0]
    V, _ = vote_counts_numpy(l)
    assert V[0, :, 0].tolist() == [[2, 0, 0, 0], [0, 2, 0, 0]]
    assert V[1, :, 0].tolist() == [[2, 0, 0, 0], [2, 0, 0, 0]]
    # tied counts in the read-out: the lowest class with the modal count
    r = vote_readout_numpy(np.array([[0, 3, 3, 1], [2, 0, 2, 2], [0, 0, 0, 5]], np.int32))
    assert r["vote_class"].tolist() == [1, 0, 3] and r["vote_class"].dtype == np.int32
    assert r["variation_ratio"].tolist() == [1.0 - 3 / 7, 1.0 - 2 / 6, 0.0]


def bad_case(scaled):
    """(clean logits, the same with bad rows, cal, the bad rows (t, e, b)): a NaN logit, a row of +inf, a -inf entry — and, ``scaled``,
    under a vector scaling an inf the scale produces from a finite logit"""
    clean, _ = make_case(3, 4, 11, 10, 3, 9)
    l = clean.copy()
    l[0, 1, 2, 3] = np.nan
    l[1, 0, 4, :] = np.inf
    l[2, 3, 5, 0] = -np.inf
    rows = [(0, 1, 2), (1, 0, 4), (2, 3, 5)]
    if not scaled:
        return clean, l, {}, rows
    l[1, 2, 7, 6] = 3e38                           # finite; times 2 it is not
    a = np.ones((4, 10), np.float32)
    a[2, 6] = 2.0
    return clean, l, dict(scale=a, bias=np.zeros((4, 10), np.float32)), rows + [(1, 2, 7)]


@pytest.mark.parametrize("scaled", [False, True], ids=["raw", "scaled"])
def test_non_finite_rows_cast_no_vote(scaled):
    clean, l, cal, rows = bad_case(scaled)
    Vc, nf0 = vote_counts_numpy(clean, **cal)
    assert nf0 == 0 and (Vc.sum(-1) == 3).all()
    with np.errstate(over="ignore"):
        V, nf = vote_counts_numpy(l, **cal)
    assert nf == len(rows)
    keep = np.ones((3, 2, 4, 11), dtype=bool)      # [t, kind, e, b]: who still votes
    for t, e, b in rows:
        keep[t, 0, e, b] = False
        keep[t, 1, e:, b] = False                  # the ensembles from the bad exit on
    assert np.array_equal(V.sum(-1), keep.sum(0))
    # the images without a bad row keep their counts
    untouched = [b for b in range(11) if b not in {r[2] for r in rows}]
    assert np.array_equal(V[:, :, untouched], Vc[:, :, untouched])
    # by hand, per pass: the clean input's per-pass votes without those of the rows that may not vote (a bad member would change the later
    # ensembles' q, but those rows do not vote at all; an ensemble row in front of it is untouched)
    per = np.stack([vote_counts_numpy(clean[t:t + 1], **cal)[0] for t in range(3)])      # [T, 2, E, B, C]
    assert np.array_equal(per.sum(0), Vc)
    assert np.array_equal(V, (per * keep[..., None]).sum(0))
    r = vote_readout_numpy(vote_counts_numpy(np.full((2, 2, 3, 4), np.nan, np.float32))[0])
    assert (r["vote_class"] == -1).all() and (r["variation_ratio"] == 1.0).all() and (r["vote_entropy"] == 0.0).all()


def test_read_out_identities():
    C_ = 12
    # unanimous
    V = np.zeros((5, C_), np.int32)
    V[np.arange(5), [0, 3, 11, 7, 7]] = [1, 2, 100, 7, 2 ** 30]
    r = vote_readout_numpy(V)
    assert r["vote_class"].tolist() == [0, 3, 11, 7, 7]
    assert (r["variation_ratio"] == 0.0).all() and (r["vote_entropy"] == 0.0).all() and not np.signbit(r["vote_entropy"]).any()
    # an even k-way split: ratio 1 - 1 / k, entropy log k
    for k in (2, 3, 5, 12):
        for each in (1, 4, 1000):
            V = np.zeros((1, C_), np.int32)
            V[0, C_ - k:] = each
            r = vote_readout_numpy(V)
            assert r["vote_class"][0] == C_ - k
            assert r["variation_ratio"][0] == 1.0 - float(each) / float(each * k)
            np.testing.assert_allclose(r["variation_ratio"][0], 1 - 1 / k, rtol=1e-15)
            np.testing.assert_allclose(r["vote_entropy"][0], np.log(k), rtol=1e-14)
    # n = 0: the sentinels, no NaN
    r = vote_readout_numpy(np.zeros((2, 3, C_), np.int32))
    assert r["vote_class"].shape == (2, 3) and (r["vote_class"] == -1).all()
    assert (r["variation_ratio"] == 1.0).all() and (r["vote_entropy"] == 0.0).all()
    # a general row against scipy-free arithmetic
    V = np.array([[5, 0, 3, 2]], np.int32)
    f = np.array([0.5, 0.3, 0.2])
    r = vote_readout_numpy(V)
    np.testing.assert_allclose(r["vote_entropy"][0], -(f * np.log(f)).sum(), rtol=1e-14)
    assert r["variation_ratio"][0] == 0.5 and r["vote_class"][0] == 0


def test_a_diagonal_matrix_gives_vector_scaling_s_votes():
    l, _ = make_case(3, 4, 13, 10, 3, 21)
    cal = make_map("vector", 4, 10, 21)
    M = np.zeros((4, 10, 10), np.float32)
    M[:, np.arange(10), np.arange(10)] = cal["scale"]
    for W in (None, make_weights(4, 21)):
        Vv, _ = vote_counts_numpy(l, weights=W, **cal)
        Vm, _ = vote_counts_numpy(l, weights=W, matrix=M, bias=cal["bias"])
        assert np.array_equal(Vv, Vm)
    assert not np.array_equal(Vv, vote_counts_numpy(l)[0])             # the scaling moves votes: the comparison is not vacuous


@pytest.mark.parametrize("kind", MAPS)
def test_one_hot_weight_rows_give_that_exit_s_classifier_votes(kind):
    l, _ = make_case(3, 4, 17, 10, 3, 22)
    cal = make_map(kind, 4, 10, 22)
    pick = [0, 0, 2, 1]                                                # row e selects exit pick[e] <= e
    W = np.zeros((4, 4))
    W[np.arange(4), pick] = 1.0
    no_equal, gap = vote_gap(l, weights=W, **cal)
    assert no_equal and gap >= GAP                                     # q_e = p_pick[e]: its arg-max is z's where the top two are apart
    V, _ = vote_counts_numpy(l, weights=W, **cal)
    assert np.array_equal(V[1], V[0][pick])
    with pytest.raises(ValueError):
        vote_counts_numpy(l, tau=1.5, scale=np.ones(10, np.float32))
