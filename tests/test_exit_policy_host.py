"""Host side of the exit-policy sweep (no GPU): the numpy restatements against the golden file pinned to the reference's confidence_exiting /
flop_saver / flop_saver_ensembled, against a scalar transcription of exit_rule_stat, the cost model of the staged engine on hand-made stage
plans, and the C ABI's validation, which is decided before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train import confidence_exiting as cex
from bayesnn_fpga_amd.train.exit_policy import (_from_ordinal, _ordinal, exit_policy_numpy, exit_stat_numpy, policy_macs, policy_metrics,
                                                reference_costs, stage_costs)
from bayesnn_fpga_amd.train.reliability import reliability_numpy
from tests.helpers import load_golden


def test_restatement_reproduces_the_reference_sweep():
    """S1 = p, t = 1: the count rows times reference_costs are flop_saver / flop_saver_ensembled as integers, sum hits / N the accuracy,
    and the rows gathered by exit_of the reference's best predictions, for both rules and all five thresholds"""
    g = load_golden("confidence_exiting.npz")
    p, labels = g["p"], g["onehot"].argmax(axis=1)
    E, N, _ = p.shape
    rec = reliability_numpy(p, labels)
    cols = np.arange(N)
    for diff, rule in ((0, "confidence"), (1, "margin")):
        stat = exit_stat_numpy(p, 1, rule)
        sw = exit_policy_numpy(stat[0], g["thresholds"], rec["keys"][:E], rec["hit"][:E], rec["nll"][:E], rec["brier"][:E], first_exit=1)
        assert not sw["invalid"].any() and (sw["count"].sum(axis=1) == N).all() and not sw["count"][:, 0].any()
        for k in range(len(g["thresholds"])):
            np.testing.assert_array_equal(p[sw["exit_of"][k].astype(np.int64), cols], g[f"best_{k}_{diff}"])
            assert sw["hits"][k].sum() / N == float(g[f"acc_{k}_{diff}"])
            if diff:
                continue                     # (the golden costs are the confidence rule's)
            for eo in (0, 1):
                for ens, name in ((False, "flops"), (True, "ensflops")):
                    costs = reference_costs("resnet18", bool(eo), 10, ensembled=ens)
                    got = policy_metrics(sw, costs, N)["cost"][k]
                    assert isinstance(got, int) and got == int(g[f"{name}_{k}_{eo}"]), (k, eo, name)
    for eo in (True, False):
        np.testing.assert_array_equal(reference_costs("resnet18", eo, 10), [cex.flops_standard_exit("resnet18", l, 10) if eo else
                                                                            10 * cex.flops_standard_exit("resnet18", l, 1) for l in range(4)])


def scalar_stat(S1, b, e, t, margin, ensemble, w):
    """exit_rule_stat of csrc/exit_rule.h, transcribed line by line for one (image, exit)"""
    E, B, Cd = S1.shape
    m1 = m2 = -1.0
    for c in range(Cd):
        if ensemble and w is not None:
            p = 0.0
            for x in range(e + 1):
                p = p + float(w[x]) * (float(S1[x, b, c]) / t)
        elif ensemble:
            acc = 0.0
            for x in range(e + 1):
                acc = acc + float(S1[x, b, c]) / t
            p = acc / float(e + 1)
        else:
            p = float(S1[e, b, c]) / t
        if p > m1:
            m2, m1 = m1, p
        elif p > m2:
            m2 = p
    return m1 - (m2 if Cd > 1 else 0.0) if margin else m1


@pytest.mark.parametrize("E,B,Cd,t,weighted", [(4, 9, 10, 7, False), (4, 9, 10, 7, True), (3, 5, 1, 3, False), (1, 4, 2, 1, True),
                                              (5, 6, 3, 10, True)])
def test_stat_restatement_equals_the_scalar_transcription(E, B, Cd, t, weighted):
    rng = np.random.RandomState(E * 100 + Cd)
    S1 = rng.dirichlet(np.ones(Cd), size=(E, B)) * t
    S1[0, 0] = S1[0, 0, ::-1].copy()
    if Cd > 1:
        S1[-1, 1, :] = t / Cd                # a tie: margin 0
        S1[0, 2, 0] = np.nan                 # a NaN class is passed over
    W = np.tril(rng.rand(E, E)) if weighted else None
    for rule in ("confidence", "margin"):
        got = exit_stat_numpy(S1, t, rule, W)
        assert got.shape == (2, E, B) and got.dtype == np.float64
        for ens in (0, 1):
            for e in range(E):
                for b in range(B):
                    want = scalar_stat(S1, b, e, float(t), rule == "margin", ens, None if W is None else W[e])
                    assert got[ens, e, b].tobytes() == np.float64(want).tobytes(), (rule, ens, e, b)
    if Cd == 1:
        np.testing.assert_array_equal(exit_stat_numpy(S1, t, "margin"), exit_stat_numpy(S1, t, "confidence"))
    with pytest.raises(ValueError):
        exit_stat_numpy(S1, t, "entropy")
    with pytest.raises(ValueError):
        exit_stat_numpy(S1[0], t)


def test_policy_restatement_edge_cases():
    """strict '>', NaN statistics and thresholds, repeated and unsorted thresholds, first_exit at both ends, invalid images"""
    E, N = 4, 6
    stat = np.array([[0.9, 0.2, 0.5, np.nan, np.inf, 0.5],
                     [0.1, 0.5, 0.5, np.nan, 0.0, 0.7],
                     [0.1, 0.6, 0.5, 0.9, 0.0, 0.2],
                     [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    keys = np.full((E, N), 0x3F000000, dtype=np.uint32)
    keys[1, 5] = 0                                           # image 5 is invalid where it leaves at exit 1
    hit = np.array([[1, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 1], [0, 0, 1, 1, 0, 0], [1, 1, 1, 0, 1, 1]], dtype=np.uint8)
    nll = np.arange(E * N, dtype=np.float64).reshape(E, N) + 1.0
    brier = -nll
    thr = np.array([0.5, np.nan, 0.5, -1.0, 2.0])
    sw = exit_policy_numpy(stat, thr, keys, hit, nll, brier, first_exit=1, select=True)
    np.testing.assert_array_equal(sw["exit_of"], [[3, 2, 3, 2, 3, 1], [3] * 6, [3, 2, 3, 2, 3, 1], [1, 1, 1, 2, 1, 1], [3] * 6])
    np.testing.assert_array_equal(sw["invalid"], [1, 0, 1, 1, 0])
    np.testing.assert_array_equal(sw["count"], [[0, 0, 2, 3], [0, 0, 0, 6], [0, 0, 2, 3], [0, 4, 1, 0], [0, 0, 0, 6]])
    np.testing.assert_array_equal(sw["hits"], [[0, 0, 1, 3], [0, 0, 0, 5], [0, 0, 1, 3], [0, 1, 1, 0], [0, 0, 0, 5]])
    np.testing.assert_array_equal(sw["selected"]["nll"][0], [19, 14, 21, 16, 23, 0])
    np.testing.assert_array_equal(sw["selected"]["keys"][3], [0x3F000000] * 5 + [0])
    np.testing.assert_array_equal(sw["selected"]["hit"][0], [1, 0, 1, 1, 1, 0])
    sw0 = exit_policy_numpy(stat, thr, keys, hit, nll, brier, first_exit=0)
    np.testing.assert_array_equal(sw0["exit_of"][0], [0, 2, 3, 2, 0, 1])
    last = exit_policy_numpy(stat, thr, keys, hit, nll, brier, first_exit=3)
    assert (last["exit_of"] == 3).all()
    part = exit_policy_numpy(stat, thr, keys, hit, nll, brier, n=3, first_exit=1, select=True)
    assert part["n"] == 3 and not part["exit_of"][:, 3:].any() and not part["selected"]["nll"][:, 3:].any()
    np.testing.assert_array_equal(part["count"].sum(axis=1) + part["invalid"], [3] * 5)
    for bad in (dict(first_exit=4), dict(first_exit=-1), dict(n=0), dict(n=7)):
        with pytest.raises(ValueError):
            exit_policy_numpy(stat, thr, keys, hit, nll, brier, **bad)


def test_policy_macs_on_hand_made_stage_plans():
    stages = [dict(prefix_macs=1000, suffix_macs=10, whole_batch_macs=0), dict(prefix_macs=500, suffix_macs=20, whole_batch_macs=100),
              dict(prefix_macs=300, suffix_macs=30, whole_batch_macs=0)]
    costs = stage_costs(stages, T=4, first_exit=1, n_exits=4)
    assert costs["stage_macs"] == [1040, 480, 420] and costs["whole_batch_macs"] == [0, 100, 0]
    assert costs["per_exit"] == [0, 1040, 1520, 1940]
    B = 10
    # stage 1 is run by 7 images, but its whole-batch op by all 10
    assert policy_macs([0, 3, 5, 2], costs, B) == 10 * 1040 + 7 * 480 + 10 * 100 + 2 * 420
    # nobody reaches stage 2: it adds nothing
    assert policy_macs([0, 3, 7, 0], costs, B) == 10 * 1040 + 7 * 480 + 10 * 100
    # everybody leaves at the first tested exit: the whole-batch op of stage 1 is not run either
    assert policy_macs([0, 10, 0, 0], costs, B) == 10 * 1040
    assert policy_macs(np.array([0, 0, 0, 10]), costs, B) == 10 * (1040 + 480 + 420) + 10 * 100
    assert isinstance(policy_macs([0, 3, 5, 2], costs, B), int)
    # without whole-batch ops the per-exit vector says the same
    plain = stage_costs([dict(s, whole_batch_macs=0) for s in stages], 4, 1, 4)
    row = [0, 3, 5, 2]
    assert policy_macs(row, plain, B) == sum(c * p for c, p in zip(row, plain["per_exit"]))
    big = stage_costs([dict(prefix_macs=2 ** 40, suffix_macs=2 ** 33, whole_batch_macs=0)], 1000, 0, 1)
    assert policy_macs([2 ** 21], big, 2 ** 21) == 2 ** 21 * (2 ** 40 + 1000 * 2 ** 33)      # beyond int64: exact Python ints
    zero = stage_costs(stages, 4, 0, 3)
    assert zero["per_exit"] == [1040, 1520, 1940]
    for row, b in (([0, 3, 5, 1], 10), ([1, 3, 5, 1], 10), ([0, 3, 5], 8), ([0, -1, 9, 2], 10)):
        with pytest.raises(ValueError):
            policy_macs(row, costs, b)
    with pytest.raises(ValueError):
        stage_costs(stages, 4, 1, 3)
    sw = dict(count=np.array([[0, 3, 5, 2], [0, 10, 0, 0]]), hits=np.array([[0, 1, 2, 2], [0, 4, 0, 0]]), invalid=np.zeros(2, dtype=np.int64), n=B)
    pm = policy_metrics(sw, costs)
    assert pm["cost"] == [policy_macs([0, 3, 5, 2], costs, B), 10 * 1040] and pm["accuracy"].tolist() == [0.5, 0.4]
    assert policy_metrics(sw, [1, 10, 100, 1000])["cost"] == [30 + 500 + 2000, 100]


def test_float64_ordinals_are_monotone_and_invertible():
    vals = [-np.inf, -1.5, -5e-324, 0.0, 5e-324, 0.5, np.nextafter(0.5, 1.0), 1.0, 1e308, np.inf]
    ords = [_ordinal(v) for v in vals]
    assert ords == sorted(set(ords)) and [_from_ordinal(o) for o in ords] == vals
    assert _ordinal(np.nextafter(0.5, 1.0)) - _ordinal(0.5) == 1 and _ordinal(-0.0) == 0


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in ("bmi_exit_stat_record", "bmi_exit_policy_sweep", "bmi_exit_policy_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert (_lib.POLICY_MAX_THRESHOLDS, _lib.POLICY_MAX_RECORD_ROWS) == (1024, 64) and _lib.POLICY_MAX_RECORD_ROWS == _lib.REL_MAX_BINS
    sb = _lib.lib().bmi_exit_policy_scratch_bytes
    chunks = lambda n: min(-(-n // 128), 128)
    assert sb(4, 10000, 11) == chunks(10000) * 11 * 9 * 4 and sb(1, 1, 1) == 12 and sb(32, 2 ** 22 - 1, 1024) == 128 * 1024 * 65 * 4
    assert sb(0, 5, 5) == sb(5, 0, 5) == sb(5, 5, 0) == sb(33, 5, 5) == sb(5, 2 ** 22, 5) == sb(5, 5, 1025) == 0


def test_c_abi_validation():
    """Every BMI_ERR_INVALID / UNSUPPORTED / NOMEM case is decided on the host before any HIP call: the output pointers here are host
    arrays, which stay as filled (a launch would never get that far without a device)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID_, UNSUPPORTED, NOMEM = -22, -95, -12
    out = np.full(2 * 4 * 103, 7.25)
    outp = C.c_void_p(out.ctypes.data)
    # bmi_exit_stat_record(S1, E, B, C, t_count, criterion, weights, n0, N_cap, stat, stream)
    ok = [fake, 4, 100, 10, 5, 0, None, 3, 103, outp, None]
    for i in (0, 9):
        args = list(ok)
        args[i] = None
        assert lib.bmi_exit_stat_record(*args) == INVALID_, i
    for i, values in ((1, (0, -1)), (2, (0, -1, 101)), (3, (0, -1)), (4, (0, -1)), (5, (2, -1)), (7, (-1, 4)), (8, (0, -1, 102))):
        for v in values:
            args = list(ok)
            args[i] = v
            assert lib.bmi_exit_stat_record(*args) == INVALID_, (i, v)
    for i, v in ((1, 33), (3, 129)):
        args = list(ok)
        args[i] = v
        assert lib.bmi_exit_stat_record(*args) == UNSUPPORTED, (i, v)
    assert (out == 7.25).all()
    # bmi_exit_policy_sweep(stat, E, N, N_cap, first_exit, thresholds, G, keys, hit, nll, brier, count, hits, invalid, exit_of,
    #                       sel_keys, sel_hit, sel_nll, sel_brier, scratch, scratch_bytes, stream)
    ints = np.full(3 * 11 * 4, -3, dtype=np.int64)
    rows = np.full(11 * 1003 * 8, 0x5A, dtype=np.uint8)
    ip, rp = C.c_void_p(ints.ctypes.data), C.c_void_p(rows.ctypes.data)
    need = lib.bmi_exit_policy_scratch_bytes(4, 1000, 11)
    ok = [fake, 4, 1000, 1003, 1, fake, 11] + [fake] * 4 + [ip, ip, ip, rp, rp, rp, rp, rp, fake, need, None]
    for i in (0, 5, 7, 8, 9, 10, 11, 12, 13, 19):
        args = list(ok)
        args[i] = None
        assert lib.bmi_exit_policy_sweep(*args) == INVALID_, i
    for some in ((15,), (16, 17), (15, 16, 18), (18,)):      # some but not all of the selected records
        args = list(ok)
        for i in some:
            args[i] = None
        assert lib.bmi_exit_policy_sweep(*args) == INVALID_, some
    for i, values in ((1, (0, -1)), (2, (0, -1, 1004)), (3, (999, 0)), (4, (-1, 4, 5)), (6, (0, -1))):
        for v in values:
            args = list(ok)
            args[i] = v
            assert lib.bmi_exit_policy_sweep(*args) == INVALID_, (i, v)
    none_selected = list(ok)
    none_selected[14:19] = [None] * 5                        # exit_of and the selected records are optional
    for change in ({1: 33, 4: 1}, {6: 1025}, {2: 2 ** 22, 3: 2 ** 22}):
        args = list(none_selected)
        for i, v in change.items():
            args[i] = v
        args[20] = 1 << 40
        assert lib.bmi_exit_policy_sweep(*args) == UNSUPPORTED, change
    args = list(ok)
    args[6], args[20] = 65, 1 << 40                          # selected records beyond 64 thresholds
    assert lib.bmi_exit_policy_sweep(*args) == UNSUPPORTED
    for short in (0, need - 1):
        for base in (ok, none_selected):
            args = list(base)
            args[20] = short
            assert lib.bmi_exit_policy_sweep(*args) == NOMEM, short
    assert (ints == -3).all() and (rows == 0x5A).all()
