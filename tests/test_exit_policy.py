"""-m gpu: the exit-policy sweep on the device (bmi_exit_stat_record, bmi_exit_policy_sweep, MCDEngine.exit_stat_records / exit_policy_sweep /
exit_costs, ExitPolicyAnalysis) — both kernels against ``exit_stat_numpy`` / ``exit_policy_numpy`` bit for bit on buffers with canaries and
spare columns, uneven record cuts, reproducibility, graph capture, errors that write nothing, the selected records through the reliability
table and the KDE, and the property the feature exists for: the sweep's exits, counts and cost ARE ``predict_early_exit``'s."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train import ExitPolicyAnalysis
from bayesnn_fpga_amd.train.exit_policy import exit_policy_numpy, exit_stat_numpy, policy_macs, policy_metrics
from bayesnn_fpga_amd.train.reliability import reliability_kde_numpy, reliability_numpy, table_metrics
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded
from tests.test_reliability_host import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind each buffer
SPARE = 3                     # columns beyond N: never written
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097)
EXITS = (1, 2, 4, 32)
FILLS = {torch.float64: -7.25, torch.int64: -7, torch.int32: -7, torch.uint8: 249}
SEL = ("sel_keys", "sel_hit", "sel_nll", "sel_brier")
SEL_DTYPES = (torch.int32, torch.uint8, torch.float64, torch.float64)
ROWS = ("keys", "hit", "nll", "brier")


class Guarded:
    """A device buffer of ``shape`` filled with its dtype's canary value, with PAD canaries in front of and behind it"""

    def __init__(self, shape, dtype):
        self.shape, self.fill = tuple(shape), FILLS[dtype]
        self.n = int(np.prod(self.shape))
        self.flat = torch.full((PAD + self.n + PAD,), self.fill, dtype=dtype, device=DEV)

    @property
    def p(self):
        return C.c_void_p(self.flat.data_ptr() + PAD * self.flat.element_size())

    def view(self):
        return self.flat[PAD:PAD + self.n].view(self.shape)

    def numpy(self):
        return self.view().cpu().numpy()

    def canaries_intact(self):
        a = self.flat.cpu().numpy()
        return bool((a[:PAD] == self.fill).all() and (a[-PAD:] == self.fill).all())

    def as_filled(self):
        return bool((self.flat.cpu().numpy() == self.fill).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the statistic record -----------------------------------------------------------------------------------------------------------
def stat_case(E, B, Cd, T, seed):
    """Sums of T softmax samples, with an all-equal row (a tie), a NaN class and infinite classes among them"""
    rng = np.random.RandomState(seed)
    S1 = rng.dirichlet(np.full(Cd, 0.3), size=(E, B)) * T
    S1[0, 0] = T / Cd
    if B > 2 and Cd > 1:
        S1[E - 1, 1, 0] = np.nan            # a NaN class is passed over
        S1[0, 2, Cd - 1] = np.inf
        if Cd > 2:
            S1[0, 2, 0] = np.inf             # two infinite classes: the margin is inf - inf, a NaN statistic
    return S1


def record_stats(S1, T, rule, W, cuts, cap):
    """bmi_exit_stat_record over the batches ``cuts`` into a guarded [2][E][cap] buffer -> the buffer"""
    E, B, Cd = S1.shape
    out = Guarded((2, E, cap), torch.float64)
    wd = None if W is None else torch.from_numpy(np.ascontiguousarray(W)).to(DEV)
    off, keep = 0, []
    for b in cuts:
        part = torch.from_numpy(np.ascontiguousarray(S1[:, off:off + b])).to(DEV)
        keep.append(part)
        rc = _lib.lib().bmi_exit_stat_record(ptr(part), E, b, Cd, T, _lib.EXIT_RULES[rule], ptr(wd), off, cap, out.p, stream())
        assert rc == _lib.BMI_OK
        off += b
    torch.cuda.synchronize()
    assert off == B
    return out


def cuts_of(B, way):
    if way == 0 or B < 3:
        return [B]
    if way == 1:
        return [B // 3, 1, B - B // 3 - 1]
    return [1] + [B - 1]


@pytest.mark.parametrize("Cd", (1, 2, 10, 128))
def test_stat_record_equals_the_numpy_restatement(Cd):
    """Every (exit, ensemble, image) against exit_stat_numpy bit for bit: both rules, with and without a weight matrix, in one call and in
    uneven cuts; spare columns and canaries untouched"""
    for i, E in enumerate(EXITS):
        sizes = SIZES if (Cd, E) == (10, 4) else (SIZES[(i + Cd) % 3], 65, 257) if E * Cd < 4096 else (3, 65)
        for j, B in enumerate(sizes):
            T = 1 + (B + E) % 7
            S1 = stat_case(E, B, Cd, T, 1000 * Cd + 10 * E + j)
            W = np.tril(np.random.RandomState(E + j).rand(E, E)) if (i + j) % 2 else None
            for rule in ("confidence", "margin"):
                want = exit_stat_numpy(S1, T, rule, W)
                got = [record_stats(S1, T, rule, W, cuts_of(B, way), B + SPARE) for way in ((0, 1) if rule == "margin" else (0, 2))]
                for g in got:
                    a = g.numpy()
                    assert g.canaries_intact() and (a[:, :, B:] == g.fill).all(), (E, B, rule)
                    assert np.array_equal(bits(a[:, :, :B]), bits(want)), (E, B, rule, int((bits(a[:, :, :B]) != bits(want)).sum()))
                if B > 2 and Cd > 2 and rule == "margin":
                    assert np.isnan(want[0, 0, 2])      # a NaN statistic is stored as it is


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------
def sweep_case(E, N, G, regime, invalid, seed):
    """(stat [E, N], thresholds [G], outcome rows): ``regime`` of the statistics — distinct, four levels, equal, and NaN / +inf sprinkled on
    any of them —, thresholds unsorted, repeated, negative, >= 1 and exactly equal to statistics; ``invalid``: none, sprinkled, a whole row"""
    rng = np.random.RandomState(seed)
    levels = np.array([0.25, 0.5, 0.75, 1.0])
    if regime == "distinct":
        stat = rng.rand(E, N)
    elif regime == "four levels":
        stat = levels[rng.randint(0, 4, size=(E, N))]
    else:
        stat = np.full((E, N), 0.5)
    if regime == "special":
        stat = rng.rand(E, N)
        stat[rng.rand(E, N) < 0.2] = np.nan
        stat[rng.rand(E, N) < 0.1] = np.inf
    pool = np.concatenate([levels, [-0.5, 0.0, 1.5, np.inf, -np.inf], stat.ravel()[:: max(1, stat.size // 7)][:7]])
    thr = pool[rng.randint(0, len(pool), size=G)]
    if G >= 11:
        thr[:5] = [0.5, -0.5, 0.5, 1.0, np.nan]              # a repeat, a negative one, one at 1, a NaN
    keys = rng.randint(1, 0x3F800000, size=(E, N)).astype(np.uint32)
    if invalid == "sprinkled":
        keys[rng.rand(E, N) < 0.15] = 0
    elif invalid == "row":
        keys[E // 2] = 0
    hit = ((rng.rand(E, N) < 0.6) & (keys != 0)).astype(np.uint8)
    nll, brier = np.where(keys != 0, rng.rand(E, N) * 5, 0.0), np.where(keys != 0, rng.rand(E, N), 0.0)
    return stat, thr, dict(keys=keys, hit=hit, nll=nll, brier=brier)


class SweepBuffers:
    def __init__(self, E, N, G, select, exit_of=True):
        self.E, self.N, self.G, self.cap = E, N, G, N + SPARE
        cap = self.cap
        self.inp = dict(stat=Guarded((E, cap), torch.float64), thr=Guarded((G,), torch.float64), keys=Guarded((E, cap), torch.int32),
                        hit=Guarded((E, cap), torch.uint8), nll=Guarded((E, cap), torch.float64), brier=Guarded((E, cap), torch.float64))
        self.out = dict(count=Guarded((G, E), torch.int64), hits=Guarded((G, E), torch.int64), invalid=Guarded((G,), torch.int64))
        if exit_of:
            self.out["exit_of"] = Guarded((G, cap), torch.uint8)
        if select:
            self.out.update({k: Guarded((G, cap), dt) for k, dt in zip(SEL, SEL_DTYPES)})
        self.scratch = torch.empty(max(1, _lib.lib().bmi_exit_policy_scratch_bytes(E, N, G)), dtype=torch.uint8, device=DEV)

    def put(self, stat, thr, rows):
        N = self.N
        self.inp["stat"].view()[:, :N] = torch.from_numpy(stat).to(DEV)
        self.inp["thr"].view()[:] = torch.from_numpy(thr).to(DEV)
        self.inp["keys"].view()[:, :N] = torch.from_numpy(rows["keys"].view(np.int32)).to(DEV)
        for k in ("hit", "nll", "brier"):
            self.inp[k].view()[:, :N] = torch.from_numpy(rows[k]).to(DEV)

    def args(self, first_exit):
        i, o = self.inp, self.out
        p = lambda k: o[k].p if k in o else None
        return dict(stat=i["stat"].p, E=self.E, N=self.N, N_cap=self.cap, first_exit=first_exit, thresholds=i["thr"].p, G=self.G, keys=i["keys"].p,
                    hit=i["hit"].p, nll=i["nll"].p, brier=i["brier"].p, count=p("count"), hits=p("hits"), invalid=p("invalid"),
                    exit_of=p("exit_of"), sel_keys=p("sel_keys"), sel_hit=p("sel_hit"), sel_nll=p("sel_nll"), sel_brier=p("sel_brier"),
                    scratch=ptr(self.scratch), scratch_bytes=self.scratch.numel())

    def run(self, fe, **change):
        """bmi_exit_policy_sweep with first_exit = ``fe``; ``change``: arguments replaced by name -> the return code"""
        a = self.args(fe)
        a.update(change)
        rc = _lib.lib().bmi_exit_policy_sweep(*a.values(), stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        """(the outputs in columns 0 .. N-1, whether every canary and spare column is as filled)"""
        got, intact = {}, True
        for k, g in self.out.items():
            a = g.numpy()
            intact &= g.canaries_intact()
            if k == "exit_of" or k in SEL:
                intact &= bool((a[:, self.N:] == g.fill).all())
                a = a[:, :self.N]
            got[k] = a
        return got, intact


def assert_sweep_equals_restatement(buf, stat, thr, rows, first_exit, what):
    select = "sel_keys" in buf.out
    want = exit_policy_numpy(stat, thr, rows["keys"], rows["hit"], rows["nll"], rows["brier"], first_exit=first_exit, select=select)
    got, intact = buf.read()
    assert intact, what
    for k in ("count", "hits", "invalid"):
        assert np.array_equal(got[k], want[k]), (what, k)
    if "exit_of" in got:
        assert np.array_equal(got["exit_of"], want["exit_of"]), what
    if select:
        for k, name in zip(ROWS, SEL):
            assert np.array_equal(bits(got[name]), bits(want["selected"][k])), (what, name)
    assert (want["count"].sum(axis=1) + want["invalid"] == buf.N).all()
    return want


REGIMES = ("distinct", "four levels", "equal", "special")
INVALIDS = ("none", "sprinkled", "row")


@pytest.mark.parametrize("N", SIZES)
def test_sweep_equals_the_numpy_restatement(N):
    """count, hits, invalid, exit_of and the selected records against exit_policy_numpy bit for bit: every E x G (selected records up to 64
    thresholds, counts only beyond) x first_exit in {0, 1, E-1}, the regimes of statistics and invalid images taken in turn"""
    turn = SIZES.index(N)
    for E in EXITS:
        for G in (1, 11, 64, 65, 1024):
            firsts = sorted({0, min(1, E - 1), E - 1})
            if G == 1024:
                firsts = [firsts[turn % len(firsts)]]
            for fe in firsts:
                turn += 1
                regime, invalid = REGIMES[turn % 4], INVALIDS[(turn // 4) % 3]
                stat, thr, rows = sweep_case(E, N, G, regime, invalid, 7 * turn + N)
                buf = SweepBuffers(E, N, G, select=G <= 64, exit_of=G != 65)
                buf.put(stat, thr, rows)
                assert buf.run(fe) == _lib.BMI_OK
                assert_sweep_equals_restatement(buf, stat, thr, rows, fe, (N, E, G, fe, regime, invalid))


def test_strict_comparison_at_the_threshold():
    """A statistic exactly equal to the threshold does not leave; the next float64 above it does"""
    E, N = 3, 5
    stat = np.array([[0.9] * N, [0.7, np.nextafter(0.7, 1.0), np.nextafter(0.7, 0.0), 0.7, 0.2], [0.1] * N])
    rows = dict(keys=np.full((E, N), 0x3F000000, dtype=np.uint32), hit=np.ones((E, N), dtype=np.uint8), nll=np.ones((E, N)), brier=np.ones((E, N)))
    thr = np.array([0.7])
    buf = SweepBuffers(E, N, 1, select=True)
    buf.put(stat, thr, rows)
    assert buf.run(1) == _lib.BMI_OK
    want = assert_sweep_equals_restatement(buf, stat, thr, rows, 1, "ties")
    assert want["exit_of"][0].tolist() == [2, 1, 2, 2, 2]


def test_record_cuts_and_runs_give_the_same_bits():
    """Uneven cuts of N into record calls leave the same statistic bits, and so the same sweep; a second run of both gives the same bits"""
    E, N, Cd, T, G = 4, 1000, 10, 5, 11
    S1 = stat_case(E, N, Cd, T, 5)
    cap = N + SPARE
    stats = [record_stats(S1, T, "confidence", None, cuts, cap) for cuts in ([N], [N], [333, 1, 600, 66], [7] * 142 + [6])]
    base = stats[0].numpy()
    assert all(np.array_equal(bits(s.numpy()), bits(base)) for s in stats[1:])
    _, thr, rows = sweep_case(E, N, G, "distinct", "sprinkled", 3)
    thr[5:] = np.quantile(base[0][:, :N][np.isfinite(base[0][:, :N])], np.linspace(0.1, 0.9, G - 5))
    outs = []
    for s in (stats[0], stats[2], stats[2]):
        buf = SweepBuffers(E, N, G, select=True)
        buf.put(s.numpy()[0][:, :N], thr, rows)
        assert buf.run(1) == _lib.BMI_OK
        outs.append(buf.read()[0])
    assert_sweep_equals_restatement(buf, base[0][:, :N], thr, rows, 1, "cuts")
    for o in outs[1:]:
        assert all(np.array_equal(bits(o[k]), bits(outs[0][k])) for k in outs[0])
    assert len({int(v) for v in outs[0]["count"][:, 1]}) > 1         # (the thresholds do cut the images differently)


def test_errors_write_nothing():
    """Every error of both calls on real device buffers: the return code, and every output as filled"""
    INVALID_, UNSUPPORTED, NOMEM = -22, -95, -12
    lib = _lib.lib()
    E, B, Cd, cap = 4, 100, 10, 103
    S1 = torch.from_numpy(stat_case(E, B, Cd, 3, 0)).to(DEV)
    out = Guarded((2, E, cap), torch.float64)
    ok = dict(S1=ptr(S1), E=E, B=B, C=Cd, t_count=3, criterion=0, weights=None, n0=3, N_cap=cap, stat=out.p)
    cases = [(dict(S1=None), INVALID_), (dict(stat=None), INVALID_), (dict(E=0), INVALID_), (dict(B=0), INVALID_), (dict(C=0), INVALID_),
             (dict(t_count=0), INVALID_), (dict(n0=-1), INVALID_), (dict(n0=4), INVALID_), (dict(criterion=2), INVALID_),
             (dict(criterion=-1), INVALID_), (dict(E=33), UNSUPPORTED), (dict(C=129), UNSUPPORTED)]
    for change, code in cases:
        a = dict(ok)
        a.update(change)
        assert lib.bmi_exit_stat_record(*a.values(), stream()) == code, change
    torch.cuda.synchronize()
    assert out.as_filled()
    N, G = 300, 11
    stat, thr, rows = sweep_case(E, N, G, "distinct", "none", 1)
    buf = SweepBuffers(E, N, G, select=True)
    buf.put(stat, thr, rows)
    cases = [(dict(stat=None), INVALID_), (dict(thresholds=None), INVALID_), (dict(keys=None), INVALID_), (dict(hit=None), INVALID_),
             (dict(nll=None), INVALID_), (dict(brier=None), INVALID_), (dict(count=None), INVALID_), (dict(hits=None), INVALID_),
             (dict(invalid=None), INVALID_), (dict(scratch=None), INVALID_), (dict(sel_keys=None), INVALID_),
             (dict(sel_hit=None, sel_nll=None), INVALID_), (dict(sel_keys=None, sel_hit=None, sel_nll=None), INVALID_), (dict(E=0), INVALID_),
             (dict(N=0), INVALID_), (dict(G=0), INVALID_), (dict(N=N + SPARE + 1), INVALID_), (dict(first_exit=-1), INVALID_),
             (dict(first_exit=E), INVALID_), (dict(E=33), UNSUPPORTED), (dict(G=1025), UNSUPPORTED), (dict(G=65), UNSUPPORTED),
             (dict(N=2 ** 22, N_cap=2 ** 22), UNSUPPORTED), (dict(scratch_bytes=0), NOMEM), (dict(scratch_bytes=buf.scratch.numel() - 1), NOMEM)]
    for change, code in cases:
        assert buf.run(1, **change) == code, change
    assert all(g.as_filled() for g in buf.out.values())
    assert buf.run(1) == _lib.BMI_OK and not buf.out["count"].as_filled()


# ---- the engine's methods -----------------------------------------------------------------------------------------------------------
KW = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)


def _model(kw=KW, dtype="f16x2"):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    m.engine_dtype = dtype
    return m


_shared = {}


def engine():
    """One engine for the tests that need the methods only (max_batch 24, as the property test runs it)"""
    if "eng" not in _shared:
        _shared["eng"] = MCDEngine(_model(dtype="f16"), DEV, max_batch=24, dtype="f16")
    return _shared["eng"]


def device_records(eng, p, y, T=1):
    """(reliability records, statistic records) of mean probabilities p [E, N, C] taken as the sums of one sample"""
    E, N, _ = p.shape
    rel, st = eng.new_reliability_records(N + SPARE), eng.new_exit_stat_records(N + SPARE)
    pd = torch.from_numpy(p).to(DEV)
    assert eng.reliability_records(pd, torch.from_numpy(y), rel, 0) == N
    assert eng.exit_stat_records(pd, T, st, 0) == N
    return rel, st


def test_selected_records_through_the_table_and_the_kde():
    """The selected records of three thresholds, handed to reliability_table and reliability_kde, give reliability_numpy /
    reliability_kde_numpy of the predictions gathered on the host — per exit and for the exit ensembles"""
    eng = engine()
    p, y = make_case(4, 1000, 10, 3, 21, 0.0)
    E, N, _ = p.shape
    rel, st = device_records(eng, p, y)
    whole = reliability_numpy(p, y)
    keys = np.ascontiguousarray(rel["keys"][:, :N].cpu().numpy()).view(np.uint32)
    assert np.array_equal(keys, whole["keys"])
    ens_rows, acc = [], np.zeros_like(p[0])
    for e in range(E):
        acc = acc + p[e]
        ens_rows.append(acc / float(e + 1))
    cols = np.arange(N)
    for ens, src in ((False, p), (True, np.stack(ens_rows))):
        stat = exit_stat_numpy(p, 1, "confidence")[int(ens)]
        assert np.array_equal(bits(st["stat"][int(ens)][:, :N].cpu().numpy()), bits(stat))
        thr = [float(np.quantile(stat[1:3], q)) for q in (0.3, 0.6, 0.9)]
        sw = eng.exit_policy_sweep(st, rel, N, thr, ensemble=ens, select=True, exit_of=True)
        ex = sw["exit_of"][:, :N].cpu().numpy().astype(np.int64)
        assert sorted(np.unique(ex).tolist()) == [1, 2, 3]
        best = np.stack([src[ex[g], cols] for g in range(3)])               # [G, N, C]: the gathered predictions, one "exit" per threshold
        want = reliability_numpy(best, y)
        table = eng.reliability_table(sw["selected"], N, 15, "mass")
        sel_keys = np.ascontiguousarray(sw["selected"]["keys"][:, :N].cpu().numpy()).view(np.uint32)
        assert np.array_equal(sel_keys, want["keys"][:3])
        assert np.array_equal(table["edges"].cpu().numpy().view(np.uint32), want["edges"][:3].view(np.uint32))
        for k in ("count", "hits", "conf_fix"):
            assert np.array_equal(table[k].cpu().numpy(), want[k][:3]), k
        np.testing.assert_allclose(table["nll_sum"].cpu().numpy(), want["nll_sum"][:3], rtol=1e-12, atol=0)
        np.testing.assert_allclose(table["brier_sum"].cpu().numpy(), want["brier_sum"][:3], rtol=1e-12, atol=0)
        assert np.array_equal(sw["hits"].sum(dim=1).cpu().numpy(), want["hit"][:3].sum(axis=1))
        kd = eng.reliability_kde(sw["selected"], N, 2 ** 10)
        kw = reliability_kde_numpy(want["keys"][:3], want["hit"][:3], N, 2 ** 10)
        for k in ("ece_kde", "bw", "sd", "n_data", "n_hit", "degenerate", "density"):
            assert np.array_equal(bits(kd[k].cpu().numpy()), bits(kw[k])), k
    with pytest.raises(ValueError):
        eng.exit_policy_sweep(st, rel, N, np.linspace(0, 1, 65), select=True)
    with pytest.raises(ValueError):
        eng.exit_policy_sweep(st, rel, N + SPARE + 1, [0.5])
    with pytest.raises(ValueError):
        eng.exit_policy_sweep(st, rel, N, [0.5], first_exit=4)
    with pytest.raises(ValueError):
        eng.exit_stat_records(torch.from_numpy(p).to(DEV), 1, st, 4)
    with pytest.raises(ValueError):
        eng.exit_stat_records(torch.from_numpy(p).to(DEV), 1, st, 0, rule="entropy")


def test_graph_capture_replays_the_same_bits():
    """ONE capture of the statistic record and the sweep (no parallel branches: one stream, three launches): the replay gives the eager bits,
    also on new inputs"""
    eng = engine()
    p, y = make_case(4, 250, 10, 3, 0, 0)
    E, N, _ = p.shape
    rel, st = device_records(eng, p, y)
    thr = torch.tensor([0.9, 0.3, 0.6, 0.6, 2.0], dtype=torch.float64, device=DEV)
    names = ("count", "hits", "invalid", "exit_of")
    eager = eng.exit_policy_sweep(st, rel, N, thr, select=True, exit_of=True)
    eager = {**{k: eager[k].clone() for k in names}, **{k: eager["selected"][k].clone() for k in ROWS}}
    ps = torch.from_numpy(p).to(DEV)
    out = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.exit_stat_records(ps, 1, st, 0)
        out.update(eng.exit_policy_sweep(st, rel, N, thr, select=True, exit_of=True))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in names) and all(torch.equal(out["selected"][k], eager[k]) for k in ROWS)
    p2 = make_case(4, 250, 10, 2, 9, 0)[0]
    ps.copy_(torch.from_numpy(p2))
    graph.replay()
    torch.cuda.synchronize()
    stat2 = exit_stat_numpy(p2, 1, "confidence")
    assert np.array_equal(bits(st["stat"][:, :, :N].cpu().numpy()), bits(stat2))
    rows = {k: rel[k][:E, :N].cpu().numpy() for k in ROWS}
    want = exit_policy_numpy(stat2[0], thr.cpu().numpy(), rows["keys"], rows["hit"], rows["nll"], rows["brier"], first_exit=1, select=True)
    for k in names:
        assert np.array_equal(out[k].cpu().numpy()[..., :N] if k == "exit_of" else out[k].cpu().numpy(), want[k][..., :N] if k == "exit_of" else want[k]), k
    for k in ROWS:
        got = out["selected"][k][:, :N].cpu().numpy()
        assert np.array_equal(bits(got), bits(want["selected"][k][:, :N])), k


def test_the_sweep_is_predict_early_exit():
    """The seeded ResNet-18 with exit-only dropout, B = 24, T = 4, C = 10: for both rules x ensemble in {False, True} and three thresholds at
    quantiles of the recorded statistics, exit_of[g] IS predict_early_exit's exit_layer, policy_macs of the count row IS its macs_done, and
    the accuracy from the hits is that of its best_preds.  Every exit from first_exit on is taken under some threshold, or the test fails."""
    # (synthetic weights of seed 1 and images of seed 0: under every rule some image is more confident at exit 2 than at exit 1, so
    # exit 2 can be taken at all; with the weights of seed 0 the exit ensembles' statistic only falls from exit 1 to exit 2)
    eng = MCDEngine(synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 1).to(DEV).eval(), DEV, max_batch=24, dtype="f16")
    B, T, seed = 24, 4, 13
    x, y = synthetic_images(B, seed=0).to(DEV), synthetic_labels(B, 10, seed=6)
    E = eng.n_exits
    S = eng.new_moments(B)
    eng.accumulate(x, S, 0, T, seed)
    rel = eng.new_reliability_records(B)
    eng.reliability_records(eng.finalize(S, T)["mean"], y, rel, 0)
    costs = eng.exit_costs(T)
    assert costs["per_exit"][0] == 0 and costs["per_exit"][E - 1] + sum(costs["whole_batch_macs"]) == costs["macs_full"]
    labels = y.numpy()
    for rule in ("confidence", "margin"):
        st = eng.new_exit_stat_records(B)
        eng.exit_stat_records(S, T, st, 0, rule)
        host = exit_stat_numpy(S[0].cpu().numpy(), T, rule)
        assert np.array_equal(bits(st["stat"].cpu().numpy()), bits(host))
        for ens in (False, True):
            # three order statistics of the recorded statistics: the lower quartile of exit 1's (images leave at exit 1), the exit-1
            # statistic of the image whose exit-2 statistic exceeds it by most (it stays at exit 1 by the strict rule and leaves at exit 2),
            # and the median of the images' largest tested statistic (the lower half goes on to the last exit)
            s = host[int(ens)]
            assert E == 4
            thr = [float(np.quantile(s[1], 0.25, method="lower")), float(s[1, np.argmax(s[2] - s[1])]),
                   float(np.quantile(s[1:E - 1].max(axis=0), 0.5, method="lower"))]
            sw = eng.exit_policy_sweep(st, rel, B, thr, ensemble=ens, select=True, exit_of=True)
            count, hits, ex = sw["count"].cpu().numpy(), sw["hits"].cpu().numpy(), sw["exit_of"].cpu().numpy()
            print(rule, ens, thr, count.tolist())
            assert not sw["invalid"].any() and (count.sum(axis=1) == B).all()
            assert (count[:, 1:].sum(axis=0) > 0).all(), f"an exit nobody takes under any of the thresholds: {count.tolist()}"
            for g, th in enumerate(thr):
                r = eng.predict_early_exit(x, T, th, seed=seed, rule=rule, ensemble=ens)
                assert np.array_equal(ex[g], r["exit_layer"].cpu().numpy()), (rule, ens, g)
                assert policy_macs(count[g], costs, B) == r["macs_done"], (rule, ens, g)
                assert hits[g].sum() / B == float((r["best_preds"].argmax(dim=1).cpu().numpy() == labels).mean()), (rule, ens, g)


def test_exit_policy_analysis_on_an_uneven_loader(tmp_path, monkeypatch):
    """Three batches of 8, 8 and 5, T = 4: ``rows`` equal exit_policy_numpy + table_metrics on host arrays of the same walk (the same
    engine, seeds seed + k), and threshold_for_budget returns the last float64 threshold whose cost fits"""
    kw = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
    m = _model(kw)
    T, seed, thr = 4, 11, (0.9, 0.2, 0.35, 0.5)
    x, y = synthetic_images(21, seed=3), synthetic_labels(21, 10, seed=4)
    loader = [(x[a:b], y[a:b]) for a, b in ((0, 8), (8, 16), (16, 21))]
    pa = ExitPolicyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, thresholds=thr, kde=True, grid_points=2 ** 10)
    eng, N, E = pa.eng, 21, pa.eng.n_exits
    assert pa.n == N and np.array_equal(pa.labels, y.numpy()) and len(pa.rows) == len(thr)
    S1, mean = [], []
    for k, (bx, _) in enumerate(loader):
        S = eng.new_moments(bx.shape[0])
        eng.accumulate(bx.to(DEV), S, 0, T, seed + k)
        S1.append(S[0].cpu().numpy())
        mean.append(eng.finalize(S, T)["mean"].cpu().numpy())
    mean = np.concatenate(mean, axis=1)
    stat = np.concatenate([exit_stat_numpy(s, T, "confidence") for s in S1], axis=2)
    assert np.array_equal(bits(pa.stat_records["stat"].cpu().numpy()), bits(stat))
    rec = reliability_numpy(mean, y.numpy())
    assert np.array_equal(np.ascontiguousarray(pa.records["keys"].cpu().numpy()).view(np.uint32), rec["keys"])
    ens_rows, acc = [], np.zeros_like(mean[0])
    for e in range(E):
        acc = acc + mean[e]
        ens_rows.append(acc / float(e + 1))
    cols = np.arange(N)
    for ens, pre, src in ((0, "", mean), (1, "ens_", np.stack(ens_rows))):
        rows = {k: rec[k][ens * E:(ens + 1) * E] for k in ROWS}
        want = exit_policy_numpy(stat[ens], np.array(thr), rows["keys"], rows["hit"], rows["nll"], rows["brier"], first_exit=1)
        best = np.stack([src[want["exit_of"][g].astype(np.int64), cols] for g in range(len(thr))])
        tm = table_metrics(reliability_numpy(best, y.numpy()))
        macs = policy_metrics(want, pa.costs, N)["cost"]
        for g, row in enumerate(pa.rows):
            assert row["threshold"] == thr[g] and row[pre + "exits"] == want["count"][g].tolist(), (pre, g)
            assert row[pre + "accuracy"] == want["hits"][g].sum() / N == tm["acc"][g] and row[pre + "ece"] == tm["ece"][g], (pre, g)
            np.testing.assert_allclose([row[pre + "nll"], row[pre + "brier"]], [tm["nll"][g], tm["brier"][g]], rtol=1e-12, atol=0)
            assert row[pre + "macs"] == macs[g] and isinstance(row[pre + "macs"], int) and 0 < row[pre + "macs_rel"] <= 1
            assert row[pre + "flops"] == sum(int(c) * int(f) for c, f in zip(want["count"][g], pa._ref_costs(bool(ens))))
    # the budget: half-way between the cheapest and the dearest policy of the grid
    for ens in (False, True):
        macs = [r[("ens_" if ens else "") + "macs"] for r in pa.rows]
        budget = (min(macs) + max(macs)) // 2
        t = pa.threshold_for_budget(budget, ensemble=ens)
        at, above = pa.policy_costs([t, float(np.nextafter(t, np.inf))], ensemble=ens)
        print(f"ensemble={ens}: budget {budget}, threshold {t!r}, cost {at}, at the next float64 {above}")
        assert at <= budget < above
    assert pa.threshold_for_budget(pa.costs["macs_full"] * N + sum(pa.costs["whole_batch_macs"]) * N) == float("inf")
    with pytest.raises(ValueError):
        pa.threshold_for_budget(pa.costs["per_exit"][1] * N - 1)
    monkeypatch.chdir(tmp_path)
    name = pa.save("t")
    lines = open(name).read().splitlines()
    assert name == "test_exit_policy_t.csv" and len(lines) == 1 + 2 * len(thr) and lines[0].startswith("Policy,Threshold,Accuracy,ECE,FLOPs_rel,NLL")
    assert lines[1].split(",")[:2] == ["E", "0.9"] and lines[2].split(",")[0] == "Ensemble"
    m.set_exit_ensemble_weights(np.ones(E))
    with pytest.raises(NotImplementedError):
        ExitPolicyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, thresholds=thr)
