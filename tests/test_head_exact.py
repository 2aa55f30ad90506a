"""Exact-logit tests of the fused exit head (csrc/head_fused_body.h) over every instantiation, through bmi_head_fused_ex.

tests/exact_head.py builds operands under which every raw logit is exact in fp32 in any summation order: SL and the per-sample `logits`
output must equal a float64 reference BIT FOR BIT in every launch form, and S1 / S2 / SH stay within bounds derived from what still rounds
(expf, the class sum, the division, logf): rtol 2e-5 (S1) and 4e-5 (S2) with atol 0, 1e-5 per sample (SH).
Every buffer sits between NaN flanks and the accumulators start from known non-zero quarter-integers.

The CPU part checks the operands (exactness in three K orders, sensitivity to the index errors the GPU part is there to catch, a
non-degenerate softmax, the guards); it checks no kernel.  The GPU part: (a) the instantiation matrix against the reference, (b) launch
forms anchored to each other with torch.equal, (c) the atomics path, (d) the K-split fallback for 3 and 4 class tiles in a child process,
(e) declines and invalid arguments.

Template parameter -> a case that launches it (ids of test_matrix unless another test is named):
    RT 1 | 2 | 3 | 4        C 1, 10, 32 | 33, 64 | 65, 96 | 100, 128: every id with that C
    KIND 0..4               -f16- | -f32- | -bf16- | -f16x2- | -bf16x3- in every id
    CSPLIT true             every C >= 65 id; the 7-mask swizzle of a short chunk: K288 (256 + 32), K32, K96, K544 (.. + 32), K1056 (.. + 32)
    CSPLIT false, RT >= 3   test_ksplit_fallback_child (BMI_HEAD_CSPLIT=0); K544 = 512 + 32 there
    ENT                     ids ending in -ent
    TEMP 0 | 1 | 2 | 3      no suffix | -temp | -vec | -mat
    one head | pack         single-.. | pack3-..; packs of 2, 5 and 8: test_pack_equals_single_launches
    part / join             tc 33, 64, 70 ids (scratch); gridDim.y == 1: tc <= 32; atomics: test_atomics_path
    imap, join over imap    test_image_map (tc = 8 and tc = 70)
    b0 / elem_off           test_image_offset
    logits only, tstride    test_logits_only_and_stride

Largest observed error as a fraction of its bound over the whole GPU part on an MI355X (test_zz_error_fractions prints them):
    S1 0.027, S2 0.108, SH 0.100."""
import ctypes
import functools
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from tests import exact_head as xh
from tests.exact_head import HeadCase
from tests.exact_ops import Guarded, roundtrip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
MATRIX = xh.matrix_cases()
OK = _lib.BMI_OK


# ---- the cases of parts (b), (c) and (e): module constants, so that the CPU part checks their operands too ---------------------------------
def _pack(n):
    """n heads that differ in K, HW, site, weights and det; tc = 33: two groups, the pack's join."""
    base = HeadCase(C=37, K=32, HW=1, B=3, tc=33, ent=True, cal="vec")
    return [xh._with_site(replace(base, K=xh.KS[h % 5], HW=xh.HWS[h % 4], det=bool(h % 2), seed=10 + h), xh.SITES[h % 5]) for h in range(n)]


PACKS = {n: _pack(n) for n in (2, 5, 8)}
IMAP_CASES = [HeadCase(C=37, K=96, HW=4, B=5, tc=tc, site="elem", ent=True, cal="mat", seed=21) for tc in (8, 70)]
KIND_BASE = HeadCase(C=100, K=288, HW=4, B=2, tc=33, site="msk", ent=True, cal="vec", seed=22)
ONE_BASES = [HeadCase(C=C_, K=96, HW=4, B=2, tc=9, site="elem", ent=True, seed=23) for C_ in (10, 70)]
PERM_BASE = HeadCase(C=37, K=96, HW=1, B=3, tc=8, site="chan", cal="mat", seed=24)
OFFSET_BASES = [xh._with_site(HeadCase(C=37, K=96, HW=4, B=5, tc=tc, ent=True, seed=25), s) for s in ("elem", "lsite") for tc in (8, 40)]
LOGITS_BASE = HeadCase(C=65, K=288, HW=4, B=3, tc=33, site="elem", cal="temp", ent=True, seed=26)
ATOMICS = [xh._with_site(HeadCase(C=C_, K=K, HW=hw, B=3, tc=tc, kind=kind, ent=ent, cal=cal, scratch=False, seed=27), s)
           for (C_, K, hw, tc, kind, ent, cal, s) in [(10, 96, 4, 33, "f16", True, None, "elem"), (33, 288, 1, 70, "bf16", False, "temp", "lsite"),
                                                      (65, 544, 12, 70, "f32", True, "vec", "msk"), (100, 288, 16, 33, "f16x2", True, "mat", "chan"),
                                                      (128, 32, 4, 70, "bf16x3", False, None, None)]]
DECLINE_BASE = HeadCase(C=10, K=96, HW=4, B=3, tc=8, site="elem", ent=True, seed=28)


def _all_heads():
    """every committed head (deduplicated by what its reference depends on)."""
    heads = [h for _, hs in MATRIX for h in hs] + [h for p in PACKS.values() for h in p] + IMAP_CASES + [KIND_BASE] + ONE_BASES + OFFSET_BASES + \
        [PERM_BASE, LOGITS_BASE, DECLINE_BASE] + ATOMICS + [replace(PERM_BASE, cal_form=f) for f in ("perm", "permT", "diag")] + \
        [replace(b, B=3, image_offset=2) for b in OFFSET_BASES]
    seen, out = set(), []
    for h in heads:
        key = (xh._core(h), h.site, h.site_logits, h.image_offset, h.cal, h.cal_form)
        if key not in seen:
            seen.add(key)
            out.append(h)
    return out


ALL_HEADS = _all_heads()


# ======================================================= CPU part: the operands =======================================================
def _linear32(f, w, bias, order):
    """float32 Linear with the products of every class added in the K order `order` (a permutation of range(K)); the zero weights are
    skipped: adding an exact zero changes no partial sum.  Step j adds the j-th nonzero term of every class at once."""
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    f32, w32 = f.float().numpy(), w.float().numpy()
    nz = [np.nonzero(row)[0] for row in w32]
    n = max(len(pos) for pos in nz)
    idx, wv = np.zeros((len(nz), n), dtype=np.int64), np.zeros((len(nz), n), dtype=np.float32)      # (a class with fewer terms: exact zeros at its end)
    for c, pos in enumerate(nz):
        pos = pos[np.argsort(rank[pos])]
        idx[c, :len(pos)], wv[c, :len(pos)] = pos, w32[c, pos]
    out = np.zeros((f32.shape[0], len(nz)), dtype=np.float32)
    for j in range(n):
        out = out + f32[:, idx[:, j]] * wv[None, :, j]
    return torch.from_numpy(out + bias.float().numpy()[None, :])


def _map32(o, l):
    """the kernel's calibration arithmetic restated in float32, every operation rounded."""
    l32 = l.float()
    if o["mat"] is not None:
        m, z = o["mat"].float(), None
        for j in range(l32.shape[-1]):
            term = l32[..., j:j + 1] * m[:, j]
            z = term if z is None else z + term
        return z + o["mat_bias"].float()
    if o["vec_scale"] is not None:
        return l32 * o["vec_scale"].float() + o["vec_bias"].float()
    return l32 * torch.tensor(o["inv_tau"], dtype=torch.float32) if o["inv_tau"] else l32


def test_matrix_covers_every_value():
    """every combination once, and each K, HW, tc, site value and both input forms with every class-tile count AND every calibration state."""
    combos = [(h[0].C, h[0].kind, h[0].ent, h[0].cal, len(h)) for _, h in MATRIX]
    assert len(set(combos)) == len(combos) == 9 * 5 * 2 * 4 * 2
    assert len({cid for cid, _ in MATRIX}) == len(MATRIX)
    for rt in (1, 2, 3, 4):
        for cal in xh.CALS:
            hs = [h[0] for _, h in MATRIX if h[0].rt == rt and h[0].cal == cal]
            assert {h.K for h in hs} == set(xh.KS) and {h.HW for h in hs} == set(xh.HWS) and {h.tc for h in hs} == set(xh.TCS)
            assert {("lsite" if h.site_logits else h.site) for h in hs} == set(xh.SITES) and {h.det for h in hs} == {False, True}
    for _, hs in MATRIX:
        assert all(h.t0 > 0 and h.B <= 5 and h.tc <= 70 and h.K <= 1056 and h.HW <= 16 for h in hs) and xh.CNT0 > 0
        if len(hs) > 1:
            assert len({h.K for h in hs}) == len({h.HW for h in hs}) == len({h.seed for h in hs}) == 3 and len({h.det for h in hs}) == 2
            assert len({(h.site, h.site_logits) for h in hs}) == 3


def test_pooled_values_are_exact():
    """relu + mean in the kernel's float32 arithmetic, pixels in order, is the float64 value for every committed HW — 12 included, where
    fl32(1 / 12) is not 1 / 12: the pixel sums are multiples of 12 and fl32(12 v * fl32(1 / 12)) = v."""
    assert {h.HW for h in ALL_HEADS} >= set(xh.HWS)
    for hw in sorted({h.HW for h in ALL_HEADS}):
        for h in [h for h in ALL_HEADS if h.HW == hw][:6]:
            x = xh.head_operands(h)["x"]
            assert torch.equal(xh.pooled32(x).double(), xh.pooled64(x)), h.id
            for kind in xh.KINDS:
                assert torch.equal(roundtrip(x, kind), x)
    x12 = xh.head_operands(next(h for h in ALL_HEADS if h.HW == 12))["x"]
    assert float(xh.pooled64(x12).max()) == 1.0 and float(x12.max()) == 2.0 and float((x12 < 0).sum()) > 0 and len(torch.unique(x12[:, :, :, 0])) > 2


def _exactness(h, o, f, l, z):
    """float32 Linear in three K orders — forward, reversed, four interleaved quarters — gives identical bits and the float64 value; the sum of
    the absolute terms stays far below 2^24 units of the common 2^-6 grid (so any other grouping is exact too); z under each map is exact."""
    K, f2 = h.K, f.reshape(-1, h.K)
    lin64 = f2 @ o["w"].T + o["bias"]
    for order in (np.arange(K), np.arange(K)[::-1].copy(), np.concatenate([np.arange(q, K, 4) for q in range(4)])):
        assert torch.equal(_linear32(f2, o["w"], o["bias"], order).double(), lin64), h.id
    grid = (f2.abs() @ o["w"].abs().T + o["bias"].abs()) * 64
    assert torch.equal(lin64 * 64, torch.round(lin64 * 64)) and float(grid.max()) < 2 ** 16, h.id
    assert torch.equal(l.float().double(), l) and torch.equal(_map32(o, l).double(), z), h.id
    if o["mat"] is not None:      # every partial sum of a matrix row on the 2^-7 grid and small: exact in any order
        assert float((l.abs() @ o["mat"].abs().T).max()) * 128 < 2 ** 16, h.id


def _changed(a, b):
    return (a != b).flatten(0, -2).any(-1)


def _sensitive(h, changed):
    """Does the wrong index show?  No choice of operands makes EVERY sample show a swap of two channels or two classes: a sample whose two
    pooled values (or logits) are equal, or both dropped by the site, computes the same logits either way, and with up to 350 samples of
    small integers some always are.  One differing logit is what the GPU part needs — it compares every logit of every sample bit for
    bit — so that is the condition; with more than one image, every image must have such a sample."""
    per_image = changed.reshape(h.tc, h.B).any(0)
    return bool(per_image.all()) if h.tc >= 8 else bool(changed.any())


def _sensitivity(h, o, f, l, z):
    K, w = h.K, o["w"]
    # two feature channels swapped: different 8-channel groups, different 256-chunks where K allows
    # (swapping columns k1 and k2 of w changes logit c of a sample by (w[c,k1] - w[c,k2]) * (f[k2] - f[k1]), one exact product, times the
    #  logits site's multiplier: all k2 of one k1 at once)
    ks = torch.arange(K)
    lm = xh.logits_site64(h)
    ok = False
    for k1 in np.nonzero(w.abs().sum(0).numpy())[0][:16].tolist():
        dw = (w[:, k1:k1 + 1] != w).double()                                                   # [C, K]
        vis = (dw.sum(0) > 0).expand(h.tc, h.B, K) if lm is None else ((lm != 0).double() @ dw) > 0
        changed = vis & (f != f[..., k1:k1 + 1])                                                # [tc, B, K]
        allowed = (ks // 8 != k1 // 8) & ((ks // 256 != k1 // 256) if K > 256 else torch.ones(K, dtype=torch.bool))
        cand = ks[allowed][:64]
        shows = changed[..., cand].any(0).all(0) if h.tc >= 8 else changed[..., cand].any(0).any(0)      # (_sensitive for every candidate)
        if bool(shows.any()):
            k2 = int(cand[shows][0])
            w2 = w.clone()
            w2[:, [k1, k2]] = w[:, [k2, k1]]
            assert _sensitive(h, _changed(xh.logits64(h, o, f, w=w2), l))                      # (the reference itself agrees)
            ok = True
            break
    assert ok, f"{h.id}: no channel swap shows"
    if h.C >= 2:      # two classes swapped (weights and bias: the class index of the tile, the bias or the join)
        pre = f @ w.T + o["bias"]                                                              # before the logits site
        ok = False
        for c1 in range(h.C - 1):
            for c2 in range(c1 + 1, min(h.C, c1 + 5)):
                differ = pre[..., c1] != pre[..., c2]
                if lm is not None:
                    differ = differ & ((lm[..., c1] != 0) | (lm[..., c2] != 0))
                if _sensitive(h, differ.flatten()):
                    pm = torch.arange(h.C)
                    pm[c1], pm[c2] = c2, c1
                    assert _sensitive(h, _changed(xh.logits64(h, dict(o, bias=o["bias"][pm]), f, w=w[pm]), l))
                    ok = True
                    break
            if ok:
                break
        assert ok, f"{h.id}: no class swap shows"
    if h.site in ("elem", "chan") or (h.site == "msk" and h.tc > 1):      # the draw of the sample before (tc = 1: of the image before)
        assert _sensitive(h, _changed(xh.logits64(h, o, xh.features64(h, o, shift_site=True)), l)), f"{h.id}: the neighbour's site draw does not show"
    if h.cal == "mat" and h.cal_form in ("rand", "perm") and h.C >= 2:
        assert _sensitive(h, _changed(l @ o["mat"] + o["mat_bias"], z)), f"{h.id}: the transposed matrix does not show"


def _softmax(h, o, f, l, z):
    """the median top-1 probability is below 0.9 and max z - min z <= 16 (C = 1 has one probability, 1: only the range applies)."""
    assert float((z.max(-1).values - z.min(-1).values).max()) <= 16.0, h.id
    if h.C > 1:
        assert float(torch.softmax(z, -1).max(-1).values.flatten().median()) < 0.9, h.id


@functools.lru_cache(maxsize=None)
def _operand_findings():
    """One walk over every committed head — in the order of what the operands depend on, so that heads which share them find them cached —
    for the three conditions below: the features, logits and z of a head are computed once.  Returns {condition: [failure, ..]}."""
    found = dict(exactness=[], sensitivity=[], softmax=[])
    checks = dict(exactness=_exactness, sensitivity=_sensitivity, softmax=_softmax)
    for h in sorted(ALL_HEADS, key=lambda h: (xh._core(h), h.id)):
        o = xh.head_operands(h)
        f = xh.features64(h, o)
        l = xh.logits64(h, o, f)
        z = xh.mapped64(o, l)
        for name, check in checks.items():
            try:
                check(h, o, f, l, z)
            except AssertionError as e:
                found[name].append(str(e) or h.id)
    return found


def test_logits_are_exact_in_any_order():
    assert _operand_findings()["exactness"] == []


def test_reference_is_sensitive_to_wrong_indices():
    assert _operand_findings()["sensitivity"] == []


def test_softmax_is_not_degenerate():
    assert _operand_findings()["softmax"] == []


def test_guards_detect_a_stray_write():
    for dtype, shape in ((torch.float64, (3, 10)), (torch.float32, (8, 60))):      # an S buffer, the logits
        for where in (-1, None):
            g = Guarded(shape, dtype, "cpu", 1, int(np.prod(shape[1:])))
            assert g.flanks_intact()
            idx = g.flank - 1 if where == -1 else g.flank + g.body.numel()
            g.buf[idx] = 0.25
            assert not g.flanks_intact()
    g = xh.guarded(torch.tensor([4, 1, 2], dtype=torch.int32), "cpu", fill=xh.INT_FILL)
    assert g.flanks_intact()
    g.buf[-1] = 0
    assert not g.flanks_intact()


# ======================================================= GPU part ====================================================================
FRAC = dict(S1=0.0, S2=0.0, SH=0.0)       # the largest observed error / bound, over everything this process has run


def _check_moments(case, ref, inc, what):
    """S1 / S2 / SH increments of one launch against the float64 softmax of the exact z."""
    worst = {}
    for k in ("S1", "S2", "SH"):
        if inc.get(k) is None:
            continue
        err = (inc[k] - ref[k]).abs()
        assert not torch.isnan(err).any(), f"{what}: NaN in {k}"
        bound = xh.moment_bound(case, ref, k)
        # (a zero reference — a row the launch does not cover — has a zero bound: the increment must be exactly 0)
        frac = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        worst[k] = float(frac.max())
        FRAC[k] = max(FRAC[k], worst[k])
    print(f"{what}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"{what}: {k} is {v:.3f} of its bound"


def _bit_equal(got, want, what):
    """torch.equal, with NaN (an element the launch must leave alone) equal to NaN."""
    assert got.shape == want.shape, f"{what}: shapes {tuple(got.shape)} and {tuple(want.shape)}"
    differ = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    if bool(differ.any()):
        bad = differ.nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ, first at {bad[0].tolist()}: got {float(got[tuple(bad[0])])}, "
                             f"want {float(want[tuple(bad[0])])}; last at {bad[-1].tolist()}")


def _check_against_reference(heads, rcs, snaps, guards_ok, t0s, what):
    """the assertions of one matrix case: BMI_OK, SL and logits bit-equal, S1 / S2 / SH within their bounds, flanks intact, the second
    launch adds."""
    assert rcs == [OK] * len(t0s), f"{what}: rc = {rcs}"
    assert guards_ok, f"{what}: a flank was written"
    for hi, h in enumerate(heads):
        init = xh.acc_init(h)
        prev = dict(S1=init[0], S2=init[1], SL=init[2], SH=init[3, :, 0])
        for i, t0 in enumerate(t0s):
            ref, got = xh.head_reference(h, t0), snaps[i][hi]
            tag = f"{what} head {hi} call {i}"
            _bit_equal(got["SL"], prev["SL"] + ref["SL"], tag + " SL")
            if got["logits"] is not None:
                _bit_equal(got["logits"], ref["logits"], tag + " logits")
                assert bool(torch.isnan(got["gaps"]).all()), tag + ": the gaps of logits_tstride were written"
            inc = {k: got[k] - prev[k] for k in ("S1", "S2", "SH") if got[k] is not None}
            _check_moments(h, ref, inc, tag)
            prev = got


@gpu
@pytest.mark.parametrize("cid", [cid for cid, _ in MATRIX])
def test_matrix(cid):
    """(a) every (class count, input kind, entropy, calibration, form) once against the float64 reference, scratch given."""
    heads = dict(MATRIX)[cid]
    t0s = [heads[0].t0, xh.second_t0(heads[0])]
    rcs, snaps, guards_ok = xh.run_head(heads, t0s=t0s)
    _check_against_reference(heads, rcs, snaps, guards_ok, t0s, cid)


def _same(a, b, what, keys=("S1", "S2", "SH", "SL", "logits")):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), f"{what}: {k}"
        if a[k] is not None:
            _bit_equal(a[k], b[k], f"{what} {k}")


def _run1(case, **kw):
    rcs, snaps, guards_ok = xh.run_head(case, **kw)
    assert rcs == [OK] and guards_ok, f"{case.id}: rc = {rcs}, flanks intact: {guards_ok}"
    return snaps[0][0]


@gpu
@pytest.mark.parametrize("n", [2, 5, 8])
def test_pack_equals_single_launches(n):
    heads = PACKS[n]
    rcs, snaps, guards_ok = xh.run_head(heads)
    _check_against_reference(heads, rcs, snaps, guards_ok, [heads[0].t0], f"pack{n}")
    for hi, h in enumerate(heads):
        _same(snaps[0][hi], _run1(h), f"pack{n} head {hi} against its own launch")


@gpu
@pytest.mark.parametrize("case", IMAP_CASES, ids=lambda c: c.id)
def test_image_map(case):
    """a non-monotone subset: the mapped images equal the full launch, the others keep their accumulators and NaN logits."""
    full = _run1(case)
    mapped = replace(case, imap=(4, 1, 2))
    rcs, snaps, guards_ok = xh.run_head(mapped)
    _check_against_reference([mapped], rcs, snaps, guards_ok, [case.t0], mapped.id)
    got, init = snaps[0][0], xh.acc_init(case)
    on = [4, 1, 2]
    off = [0, 3]
    for k in ("S1", "S2", "SL", "SH"):
        _bit_equal(got[k][on], full[k][on], f"{mapped.id} {k} mapped rows")
    _bit_equal(got["logits"][:, on], full["logits"][:, on], f"{mapped.id} logits")
    for i, k in enumerate(("S1", "S2", "SL")):
        assert torch.equal(got[k][off], init[i][off]), f"{mapped.id}: {k} of an unmapped image changed"
    assert torch.equal(got["SH"][off], init[3, off, 0]) and bool(torch.isnan(got["logits"][:, off]).all())


@gpu
def test_input_kinds_agree():
    """the five input kinds on the same representable activations: the same bits."""
    ref = _run1(KIND_BASE)
    for kind in xh.KINDS[1:]:
        _same(_run1(replace(KIND_BASE, kind=kind)), ref, f"{kind} against f16")


@gpu
@pytest.mark.parametrize("base", ONE_BASES, ids=lambda c: c.id)
def test_unit_maps_change_nothing(base):
    """inv_tau = 1, scale 1 / bias 0 and the identity matrix each equal the untempered launch."""
    plain = _run1(base)
    for cal in ("temp", "vec", "mat"):
        _same(_run1(replace(base, cal=cal, cal_form="one")), plain, f"{base.id}: unit {cal}")


@gpu
def test_diagonal_and_permutation_matrices():
    """a diagonal matrix equals the vector map bit for bit; a 3-cycle permutes z exactly, so S1 is the permuted S1 of the plain launch within
    the S1 bound, and the transposed (inverse) permutation is not."""
    _same(_run1(replace(PERM_BASE, cal_form="diag")), _run1(replace(PERM_BASE, cal="vec")), "diag against vec")
    plain = _run1(replace(PERM_BASE, cal=None))
    init = xh.acc_init(PERM_BASE)[0]
    perm = xh.head_operands(PERM_BASE)["perm"]
    want = (plain["S1"] - init)[:, perm]
    for form, agrees in (("perm", True), ("permT", False)):
        case = replace(PERM_BASE, cal_form=form)
        got = _run1(case)
        _check_against_reference([case], [OK], [[got]], True, [case.t0], case.id)
        inc = got["S1"] - init
        within = bool(((inc - want).abs() <= xh.RTOL_S1 * want.abs()).all())
        assert within == agrees, f"{form}: S1 {'differs from' if agrees else 'equals'} the permuted S1"
        _same(got, plain, form, keys=("SL", "logits"))


@gpu
@pytest.mark.parametrize("base", OFFSET_BASES, ids=lambda c: c.id)
def test_image_offset(base):
    """image_offset = 2 with B = 3 equals images 2..4 of the B = 5 launch at offset 0 (C = 37: b0 * C = 74 is no multiple of 8, and the quads
    of the logits site straddle two Philox calls); for the feature site and for the logits site."""
    full = _run1(base)
    part = replace(base, B=3, image_offset=2)
    rcs, snaps, guards_ok = xh.run_head(part)
    _check_against_reference([part], rcs, snaps, guards_ok, [part.t0], part.id)
    got = snaps[0][0]
    for k in ("S1", "S2", "SL", "SH"):      # (an image starts from the same prefill in both launches: acc_init)
        _bit_equal(got[k], full[k][2:], f"{part.id} {k}")
    _bit_equal(got["logits"], full["logits"][:, 2:], f"{part.id} logits")
    if base.site_logits:
        sh = (torch.arange(2, 5)[:, None] * base.C + torch.arange(0, base.C, 4)[None, :]) & 7
        assert bool((sh > 4).any()) and (2 * base.C) % 8 != 0


@gpu
def test_logits_only_and_stride():
    """logits-only mode writes the same logits and touches no accumulator; with logits_tstride = 2 B C the gaps stay NaN."""
    full = _run1(LOGITS_BASE)
    assert LOGITS_BASE.ent and LOGITS_BASE.groups > 1 and full["scratch_unwritten"] is False
    lo = _run1(replace(LOGITS_BASE, accum=False))      # S1 = S2 = SL = null; SH and the scratch are still passed
    assert lo["S1"] is None and torch.equal(lo["SH"], xh.acc_init(LOGITS_BASE)[3, :, 0]) and lo["scratch_unwritten"] is True
    _same(lo, full, "logits only", keys=("logits",))
    wide = _run1(replace(LOGITS_BASE, tstride=2))
    _same(wide, full, "logits_tstride = 2 B C")
    assert wide["gaps"].numel() == LOGITS_BASE.tc * LOGITS_BASE.B * LOGITS_BASE.C and bool(torch.isnan(wide["gaps"]).all())
    # and without a logits output: the accumulators alone
    rcs, snaps, guards_ok = xh.run_head(replace(LOGITS_BASE, logits=False))
    _check_against_reference([replace(LOGITS_BASE, logits=False)], rcs, snaps, guards_ok, [LOGITS_BASE.t0], "no logits output")


@gpu
@pytest.mark.parametrize("case", ATOMICS, ids=lambda c: c.id)
def test_atomics_path(case):
    """(c) no scratch and more than one group: hardware float64 atomics.  SL is bit-equal (exact terms are order-free), S1 / S2 / SH within
    the bounds."""
    assert not case.scratch and case.tc in (33, 70)
    t0s = [case.t0, xh.second_t0(case)]
    rcs, snaps, guards_ok = xh.run_head(case, t0s=t0s)
    _check_against_reference([case], rcs, snaps, guards_ok, t0s, case.id)


@gpu
def test_ksplit_fallback_child(tmp_path):
    """(d) BMI_HEAD_CSPLIT=0 in one fresh child process: the K-split body for 3 and 4 class tiles, fp16 inputs, every matrix case; its
    outputs equal this process's class-split outputs bit for bit, and SL and logits equal the reference.  Nothing a launch returns tells
    which body ran: the test relies on the launch switches reading that variable (csrc/head_fused_body.h, launch_rt and launch_rt_multi) —
    were it renamed or ignored, the child would run the class split and the comparison would hold vacuously; the first assertion ties the
    name to the source."""
    with open(os.path.join(ROOT, "bayesnn_fpga_amd", "csrc", "head_fused_body.h")) as src:
        assert src.read().count('std::getenv("BMI_HEAD_CSPLIT")') == 2
    path = str(tmp_path / "ksplit.npz")
    env = dict(os.environ, BMI_HEAD_CSPLIT="0")
    proc = subprocess.run([sys.executable, "-m", "tests.exact_head", path], cwd=ROOT, env=env, timeout=600, capture_output=True, text=True)
    assert proc.returncode == 0, f"the child ended with {proc.returncode}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"
    child = np.load(path)
    n = 0
    for cid, heads in MATRIX:
        if heads[0].rt < 3 or heads[0].kind != "f16":
            continue
        n += 1
        t0s = [heads[0].t0, xh.second_t0(heads[0])]
        assert child[f"{cid}|rc"].tolist() == [OK, OK, 1], f"{cid}: child rc / guards {child[f'{cid}|rc'].tolist()}"
        rcs, snaps, guards_ok = xh.run_head(heads, t0s=t0s)
        assert rcs == [OK, OK] and guards_ok
        for i in range(2):
            for hi, h in enumerate(heads):
                for k, v in snaps[i][hi].items():
                    if isinstance(v, torch.Tensor) and k != "gaps":
                        _bit_equal(torch.from_numpy(child[f"{cid}|{i}|{hi}|{k}"]), v, f"{cid} call {i} head {hi} {k}: K split against class split")
        _check_against_reference(heads, rcs, snaps, guards_ok, t0s, cid)      # (and so the child's SL and logits equal the reference)
    assert n == 4 * 2 * 4 * 2


def _declined(cases, want, **kw):
    cases = [cases] if isinstance(cases, HeadCase) else cases
    rcs, snaps, guards_ok = xh.run_head(cases, **kw)
    assert rcs == [want], f"rc = {rcs}, expected {want}"
    assert guards_ok and all(xh.untouched(c, s) for c, s in zip(cases, snaps[0])), "a refused launch wrote to an output"


@gpu
def test_declines_and_invalid_arguments():
    """(e) each leaves every output untouched."""
    b = DECLINE_BASE
    keep = [_lib.make_site(_lib.SITE_CHANNEL, 7, 0.5)]

    def set_(**fields):
        def tweak(arr, n):
            for k, v in fields.items():
                setattr(arr[0], k, v)
        return tweak

    def chan_logits(arr, n):
        arr[0].site_logits = ctypes.pointer(keep[0])

    _declined(replace(b, C=129), xh.UNSUPPORTED)
    _declined(replace(b, K=100, site=None), xh.UNSUPPORTED)
    _declined(b, xh.UNSUPPORTED, tweak=chan_logits)
    _declined(replace(b, cal="vec"), xh.INVALID, tweak=set_(inv_tau=0.5))              # a vector map together with a temperature
    _declined(replace(b, cal="vec"), xh.INVALID, tweak=set_(vec_bias=None))            # a scale without a bias
    _declined(replace(b, cal="mat"), xh.INVALID, tweak=set_(mat_bias=None))
    _declined(replace(b, imap=(0, 1)), xh.INVALID, tweak=set_(n_mapped=b.B + 1))
    _declined(b, xh.INVALID, tweak=set_(in_mod=2 * b.B))                               # neither B nor B * tc
    _declined(b, xh.INVALID, tweak=lambda arr, n: 9)                                   # n_heads = 9
    two = [replace(b, tc=33), replace(b, tc=33, seed=29)]
    _declined(two, xh.INVALID, share_scratch=True)                                     # two heads of a pack sharing one scratch
    _declined([b, replace(b, C=12)], xh.UNSUPPORTED)                                   # a pack: differing C
    _declined([b, replace(b, imap=(0, 1))], xh.UNSUPPORTED)                            # a pack: one head with an image_map
    _declined(replace(b, B=3, image_offset=1), xh.UNSUPPORTED)                         # feature-site offset 1 * 96: no whole Philox call
    _declined(b, xh.INVALID, tweak=set_(logits_tstride=b.B * b.C - 1))                 # the samples' logits rows would overlap


@gpu
def test_zz_error_fractions():
    """prints the largest S1 / S2 / SH error seen by this process as a fraction of its bound (the figures of the module docstring)."""
    print("largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in FRAC.items()))
    assert all(v <= 1.0 for v in FRAC.values())
