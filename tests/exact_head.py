"""Exact-arithmetic operands, float64 references and guarded launches for the fused exit head (tests/test_head_exact.py).

Activations are small integers (representable in fp16, bf16 and as pair32), the pooled value of every (image, channel) is an integer or a
multiple of 1 / HW with HW a power of two (HW = 12: the pixel sum is a multiple of 12 and fl32(sum * fl32(1 / 12)) is the integer), site
multipliers are in {0, 1, 2, 4}, weights in {-1/4, 0, 1/4} and the bias a multiple of 1/4: every raw logit is a multiple of 2^-6 of small
magnitude, exact in fp32 in whatever order the MFMA, the four K-quarters or the class-split chains add the terms, so SL and the per-sample
`logits` output must equal the float64 reference bit for bit.  The calibration maps are exact too (inv_tau = 1/2; power-of-two vector scales
and quarter-integer biases; matrix entries in {-1, 0, 1/2, 1, 2}); only expf, the class sum, the division and logf round, and S1 / S2 / SH
are compared under the bounds of `moment_bound`.  A plain module like tests/exact_ops.py: no fixtures."""
import ctypes as C
import functools
from dataclasses import dataclass, replace

import numpy as np
import torch

from bayesnn_fpga_amd import _lib
from tests import gpu_helpers as gh
from tests.exact_ops import T16, guarded, guarded_like, options, roundtrip

UNSUPPORTED, INVALID = -95, -22         # BMI_ERR_UNSUPPORTED, BMI_ERR_INVALID
KINDS = ("f16", "f32", "bf16", "f16x2", "bf16x3")
SEED, CNT0 = (5 << 32) + 77, 2          # Philox seed and first Masksembles row of every launch
INT_FILL = 0x5A5A5A5A                   # the flank pattern of the int32 image maps
NNZ = 4                                 # nonzero weights per class
INV_TAU = 0.5
RTOL_S1, RTOL_S2, ATOL_SH = 2e-5, 4e-5, 1e-5      # (ATOL_SH per sample of the launch)


@dataclass(frozen=True)
class HeadCase:
    """One exit head.  site: None | "elem" (p = 0.5) | "chan" (p = 0.75) | "msk" (rows over {0, 2}) on the pooled features; site_logits:
    elementwise p = 0.5 on the logits; cal: None | "temp" | "vec" | "mat", with cal_form choosing the coefficients ("rand": the exact random
    ones; "one": the map that changes nothing; for the matrix also "diag": diag(vec_scale) with vec_bias, "perm" / "permT": a 3-cycle and its inverse);
    imap: the launch's image list or None; accum False: logits only (no S1 / S2 / SL / SH); tstride: logits_tstride in units of B * C."""
    C: int
    K: int
    HW: int = 4
    B: int = 3
    tc: int = 8
    t0: int = 3
    det: bool = False
    kind: str = "f16"
    site: str = None
    site_logits: bool = False
    cal: str = None
    cal_form: str = "rand"
    ent: bool = False
    imap: tuple = None
    image_offset: int = 0
    scratch: bool = True
    logits: bool = True
    accum: bool = True
    tstride: int = 1
    seed: int = 1

    @property
    def rt(self):
        return (self.C + 31) // 32

    @property
    def groups(self):
        return (self.tc + 31) // 32

    @property
    def id(self):
        s = f"C{self.C}-K{self.K}-hw{self.HW}-B{self.B}-tc{self.tc}-{self.kind}-{'det' if self.det else 'sto'}-{self.site or 'nosite'}"
        s += ("-lsite" if self.site_logits else "") + (f"-{self.cal}" if self.cal else "") + (f".{self.cal_form}" if self.cal and self.cal_form != "rand" else "")
        s += ("-ent" if self.ent else "") + (f"-imap{''.join(map(str, self.imap))}" if self.imap else "") + (f"-b0{self.image_offset}" if self.image_offset else "")
        s += ("" if self.scratch else "-atomics") + ("" if self.logits else "-nologits") + ("" if self.accum else "-logitsonly")
        return s + (f"-ts{self.tstride}" if self.tstride != 1 else "") + (f"-s{self.seed}" if self.seed != 1 else "")


def site_dicts(case, masks=None):
    """(feature site, logits site) in gpu_helpers' form."""
    site = None
    if case.site == "elem":
        site = dict(kind=_lib.SITE_ELEMENTWISE, site_id=6, p=0.5)
    elif case.site == "chan":
        site = dict(kind=_lib.SITE_CHANNEL, site_id=3, p=0.75)
    elif case.site == "msk":
        site = dict(kind=_lib.SITE_MASKSEMBLE, site_id=1, masks=masks)
    return site, (dict(kind=_lib.SITE_ELEMENTWISE, site_id=7, p=0.5) if case.site_logits else None)


def _activations(rng, n, HW, K):
    """[n, HW, K] small integers whose pooled value is at most 1 (with NNZ weights of 1/4, a site multiplier of at most 4 and |bias| <= 3/4
    that bounds |logit| by 4.75; test_softmax_is_not_degenerate checks max z - min z <= 16 under every map).  HW a power of two: integers in
    -2..1.  Otherwise every (image, channel) has a target v in {0, 1} and its pixels are 1 +- 1 in equal numbers (v = 1) or drawn from
    {-2, -1, 0} (v = 0): after the ReLU the pixel sum is HW * v."""
    if HW & (HW - 1) == 0:
        return rng.choice([-2.0, -1.0, 0.0, 1.0, 1.0, 1.0], size=(n, HW, K))
    assert HW % 2 == 0
    v = rng.choice([0, 1], size=(n, 1, K))
    d = np.repeat(np.array([1.0, -1.0]), HW // 2)
    delta = rng.permuted(np.broadcast_to(d[None, :, None], (n, HW, K)), axis=1)
    neg = -rng.integers(0, 3, size=(n, HW, K)).astype(np.float64)
    return np.where(v > 0, v + delta, neg)


def _core(case):
    """what the operands depend on: cases that differ in anything else (input kind, calibration, entropy, scratch, image map, outputs) share
    them, and a launch at image_offset shares the batch of image_offset + B images it is a slice of."""
    return (case.C, case.K, case.HW, case.image_offset + case.B, case.tc, case.det, case.seed)


@functools.lru_cache(maxsize=8)
def _operands(core):
    C_, K, HW, Bp, tc, det, seed = core
    rng = np.random.default_rng(seed * 1000003 + C_ * 137 + K)
    o = {}
    o["x"] = torch.from_numpy(_activations(rng, (1 if det else tc) * Bp, HW, K)).reshape(1 if det else tc, Bp, HW, K)
    w = np.zeros((C_, K))
    for c in range(C_):
        pos = rng.choice(K, size=max(NNZ, 32 // C_), replace=False)       # (a head of one or two classes gets more: its range is no concern)
        w[c, pos] = rng.choice([-0.25, 0.25], size=len(pos))
    o["w"] = torch.from_numpy(w)
    o["bias"] = torch.from_numpy(rng.integers(-3, 4, size=C_) / 4.0)
    o["masks"] = (rng.random((4, K)) < 0.5).astype(np.float32) * 2.0
    o["vec_scale"] = torch.from_numpy(rng.choice([0.25, 0.5, 1.0], size=C_))
    o["vec_bias"] = torch.from_numpy(rng.integers(-2, 3, size=C_) / 4.0)
    m = np.zeros((C_, C_))
    rows = [(1.0, 0.5), (0.5, -1.0), (0.5, 1.0), (1.0, 0.0), (0.0, 2.0)]       # (diagonal, one off-diagonal entry): a row's entries add up to 2 at most
    for c in range(C_):
        d, e = rows[rng.choice(5, p=[0.3, 0.25, 0.2, 0.15, 0.1])]
        m[c, c] = d
        if C_ > 1:
            m[c, (c + 1 + rng.integers(0, C_ - 1)) % C_] = e
    o["mat"] = torch.from_numpy(m)
    o["mat_bias"] = torch.from_numpy(rng.integers(-2, 3, size=C_) / 4.0)
    o["perm"] = torch.from_numpy(np.roll(np.arange(C_), 1) if C_ < 3 else np.concatenate([[1, 2, 0], np.arange(3, C_)]))   # a 3-cycle: no involution
    return o


def head_operands(case):
    """float64 CPU operands of `case`: x [1 or tc, B, HW, K] (this launch's images), w [C, K], bias [C], masks (Masksembles rows, numpy),
    inv_tau / vec_scale / vec_bias / mat / mat_bias of its calibration state (or None)."""
    o = dict(_operands(_core(case)))
    o["x"] = o["x"][:, case.image_offset:]
    C_ = case.C
    o["inv_tau"] = 0.0
    vs = vb = m = mb = None
    if case.cal == "temp":
        o["inv_tau"] = 1.0 if case.cal_form == "one" else INV_TAU
    elif case.cal == "vec":
        vs, vb = (torch.ones(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64)) if case.cal_form == "one" else (o["vec_scale"], o["vec_bias"])
    elif case.cal == "mat":
        mb = o["mat_bias"]
        if case.cal_form == "one":
            m, mb = torch.eye(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64)
        elif case.cal_form == "diag":
            m, mb = torch.diag(o["vec_scale"]), o["vec_bias"]
        elif case.cal_form in ("perm", "permT"):
            m = torch.zeros(C_, C_, dtype=torch.float64)
            m[torch.arange(C_), o["perm"]] = 1.0          # z_c = l_perm[c]
            m, mb = (m.T.contiguous() if case.cal_form == "permT" else m), torch.zeros(C_, dtype=torch.float64)
        else:
            m = o["mat"]
    o["vec_scale"], o["vec_bias"], o["mat"], o["mat_bias"] = vs, vb, m, mb
    return o


def pooled64(x):
    """relu then mean over the pixels, float64: [.., HW, K] -> [.., K]."""
    return torch.relu(x).sum(-2) / x.shape[-2]


def pooled32(x):
    """the kernel's own arithmetic restated in float32: pixels added in order, then fl32(fl32(sum) * fl32(1 / HW))."""
    HW = x.shape[-2]
    xs = torch.relu(x).float()
    s = torch.zeros(xs.shape[:-2] + xs.shape[-1:], dtype=torch.float32)
    for p in range(HW):
        s = s + xs[..., p, :]
    return s * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(HW), dtype=torch.float32))


def features64(case, o, t0=None, shift_site=False):
    """[tc, B, K] float64: pooled features times the feature site's multiplier (drawn for image_offset + B images, then sliced).
    shift_site: every sample takes the draw of the sample before it — of the neighbouring image where the launch has one sample — (the
    sensitivity check's wrong index)."""
    t0 = case.t0 if t0 is None else t0
    f = pooled64(o["x"]).expand(case.tc, case.B, case.K)
    site, _ = site_dicts(case, o["masks"])
    if site is not None:
        Bp = case.image_offset + case.B
        m = gh.folded_site_mask(site, Bp, case.K, 1, 1, case.tc, t0, SEED, CNT0).reshape(case.tc, Bp, case.K).double()
        m = m[:, case.image_offset:]
        if shift_site:
            m = torch.roll(m, 1, 0 if case.tc > 1 else 1)
        f = f * m
    return f


def logits64(case, o, f, w=None, t0=None):
    """raw logits [tc, B, C]: Linear, bias, then the logits site."""
    l = f @ (o["w"] if w is None else w).T + o["bias"]
    m = logits_site64(case, t0)
    return l if m is None else l * m


def logits_site64(case, t0=None):
    """[tc, B, C] multiplier of the logits site (drawn for image_offset + B images, then sliced), or None."""
    _, ls = site_dicts(case)
    if ls is None:
        return None
    Bp = case.image_offset + case.B
    m = gh.folded_site_mask(ls, Bp, case.C, 1, 1, case.tc, case.t0 if t0 is None else t0, SEED, CNT0).reshape(case.tc, Bp, case.C).double()
    return m[:, case.image_offset:]


def mapped64(o, l):
    """z of the case's calibration map, float64."""
    if o["mat"] is not None:
        return l @ o["mat"].T + o["mat_bias"]
    if o["vec_scale"] is not None:
        return l * o["vec_scale"] + o["vec_bias"]
    return l * o["inv_tau"] if o["inv_tau"] else l


def head_reference(case, t0=None):
    """float64 reference of one launch: dict with logits [tc, B, C] (NaN for the images the launch does not cover), z, p, and the INCREMENTS
    S1 / S2 / SL [B, C] and SH [B] (zero rows for the images it does not cover)."""
    o = head_operands(case)
    l = logits64(case, o, features64(case, o, t0), t0=t0)
    z = mapped64(o, l)
    p = torch.softmax(z, -1)
    h = -(p * torch.log_softmax(z, -1)).sum(-1)
    r = dict(logits=l.clone(), z=z, p=p, S1=p.sum(0), S2=(p * p).sum(0), SL=l.sum(0), SH=h.sum(0))
    if case.imap is not None:
        off = torch.ones(case.B, dtype=torch.bool)
        off[list(case.imap)] = False
        r["logits"][:, off] = float("nan")
        for k in ("S1", "S2", "SL", "SH"):
            r[k][off] = 0.0
    return r


def acc_init(case):
    """the known non-zero quarter-integers the accumulators hold before a launch: [4, B, C] for S1, S2, SL and (row 3, class 0) SH.  A
    launch at image_offset gets the rows of the batch it is a slice of, so that the same image starts from the same numbers."""
    Bp = case.image_offset + case.B
    i = torch.arange(4 * Bp * case.C, dtype=torch.float64).reshape(4, Bp, case.C)
    return (((i * 7) % 11 + 1) / 4.0)[:, case.image_offset:].contiguous()


def moment_bound(case, ref, k):
    """The largest admissible |device - reference| of the INCREMENT of S1, S2 or SH (k) of one launch.  z - max is exact, expf is within 1 ulp,
    a lane adds at most 64 terms in sequence, then one shuffle add and one division: a probability is within about 68 * 2^-24 = 4.1e-6
    relative, so rtol 2e-5 (S1) and 4e-5 (S2) with atol 0, and 1e-5 per sample for the entropy.  The increments are read from float64
    accumulators that start from the non-zero prefill; the few float64 roundings of the `+=` (one with a scratch, up to three with the
    atomics) stay well inside rtol for the committed operands, whose smallest probability is about 6e-7.  Where the reference is 0 (the
    rows a launch with an image map does not cover) the bound is 0: the increment must be exactly 0."""
    if k == "SH":
        return torch.where(ref["SH"] == 0, torch.zeros_like(ref["SH"]), torch.full_like(ref["SH"], ATOL_SH * case.tc))
    return (RTOL_S1 if k == "S1" else RTOL_S2) * ref[k].abs()


# ---- launches ---------------------------------------------------------------------------------------------------------------------
def _input(x, kind, dev):
    """[in_mod, HW, K] float64 -> the guarded device tensor of the input kind."""
    if kind in ("f16", "bf16"):
        t = x.to(T16[kind])
    elif kind == "f32":
        t = x.float()
    else:
        t = gh.pair32_encode(x.float()[:, None], T16[kind])[:, 0]
    return guarded(t.contiguous(), dev)


class _Head:
    """the guarded device buffers of one head and its bmi_head_ex."""

    def __init__(self, case, dev, share_scratch=None):
        c, o = case, head_operands(case)
        self.case = c
        f32 = lambda t: guarded(t.float().contiguous(), dev) if t is not None else None
        x = o["x"].reshape(-1, c.HW, c.K)
        assert torch.equal(roundtrip(x, c.kind), x)
        self.x = _input(x, c.kind, dev)
        wp = torch.zeros(32 * c.rt, c.K, dtype=torch.float64)
        wp[:c.C] = o["w"]
        self.w, self.bias = f32(wp), f32(o["bias"])
        self.masks = f32(torch.from_numpy(o["masks"])) if c.site == "msk" else None
        self.vs, self.vb, self.m, self.mb = f32(o["vec_scale"]), f32(o["vec_bias"]), f32(o["mat"]), f32(o["mat_bias"])
        self.imap = guarded(torch.tensor(c.imap, dtype=torch.int32), dev, fill=INT_FILL) if c.imap is not None else None
        init = acc_init(c)
        self.S = [guarded(init[i], dev) for i in range(3)] if c.accum else [None] * 3
        self.SH = guarded(init[3, :, 0].contiguous(), dev) if c.ent else None       # (given in logits-only mode too: it must stay as it is)
        self.stride = c.tstride * c.B * c.C
        self.logits = guarded_like((c.tc, self.stride), torch.float32, dev) if c.logits else None
        self.scratch = share_scratch
        if c.scratch and share_scratch is None:
            self.scratch = guarded_like((c.groups * (3 * c.B * c.C + (c.B if c.ent else 0)),), torch.float64, dev)
        site, ls = site_dicts(c, o["masks"])
        self.s1 = self.s2 = None
        if site is not None:
            self.s1 = _lib.make_site(site["kind"], site["site_id"], 0.0, 4, self.masks.body.data_ptr()) if c.site == "msk" else \
                _lib.make_site(site["kind"], site["site_id"], site["p"])
        if ls is not None:
            self.s2 = _lib.make_site(ls["kind"], ls["site_id"], ls["p"])
        self.inv_tau = o["inv_tau"]

    def guards(self):
        return [g for g in [self.x, self.w, self.bias, self.masks, self.vs, self.vb, self.m, self.mb, self.imap, *self.S, self.SH, self.logits,
                            self.scratch] if g is not None]

    def struct(self, t0):
        c, p = self.case, lambda g: (g.body.data_ptr() if g is not None else None)
        h = _lib.HeadEx()
        h.in_, h.in_is_f32, h.in_mod, h.hw, h.k = p(self.x), int(c.kind == "f32"), (c.B if c.det else c.B * c.tc), c.HW, c.K
        h.weight_pad, h.bias, h.out_dim = p(self.w), p(self.bias), c.C
        h.site = C.pointer(self.s1) if self.s1 is not None else None
        h.site_logits = C.pointer(self.s2) if self.s2 is not None else None
        h.batch, h.t0, h.tc, h.seed, h.mask_cnt0 = c.B, t0, c.tc, SEED, CNT0
        h.S1, h.S2, h.SL, h.SH = p(self.S[0]), p(self.S[1]), p(self.S[2]), p(self.SH)
        h.image_map, h.n_mapped, h.image_offset = p(self.imap), (len(c.imap) if c.imap is not None else 0), c.image_offset
        h.logits, h.logits_tstride, h.scratch = p(self.logits), self.stride, p(self.scratch)
        h.inv_tau, h.vec_scale, h.vec_bias, h.mat, h.mat_bias = self.inv_tau, p(self.vs), p(self.vb), p(self.m), p(self.mb)
        return h

    def snapshot(self):
        c = self.case
        cpu = lambda g: g.body.double().cpu().clone() if g is not None else None
        out = dict(S1=cpu(self.S[0]), S2=cpu(self.S[1]), SL=cpu(self.S[2]), SH=cpu(self.SH), logits=None, gaps=None)
        out["scratch_unwritten"] = bool(torch.isnan(self.scratch.body).all()) if self.scratch is not None else None
        if self.logits is not None:
            full = self.logits.body.double().cpu()
            out["logits"] = full[:, :c.B * c.C].reshape(c.tc, c.B, c.C).clone()
            out["gaps"] = full[:, c.B * c.C:].clone()
        return out


def kind_option(kind):
    """unit_entry_dtype for an input kind (fp32 inputs are flagged by the call itself)."""
    return _lib.DTYPES["f16" if kind == "f32" else kind]


def run_head(cases, t0s=None, tweak=None, share_scratch=False):
    """Launches the head(s) of `cases` (one case, or a list: a pack) through bmi_head_fused_ex once per entry of `t0s` (default: the case's
    own t0) on the same buffers.  tweak(structs): edits the bmi_head_ex array before every call (the invalid-argument tests).  Returns
    (rcs, snaps, guards_ok): the return codes, per call the decoded outputs of every head (S1 / S2 / SL [B, C], SH [B], logits [tc, B, C],
    gaps = what lies between the samples' logits rows, scratch_unwritten = the scratch is still all NaN), and whether every flank of every
    buffer is intact."""
    cases = [cases] if isinstance(cases, HeadCase) else list(cases)
    dev, lib = gh.DEV, _lib.lib()
    heads = []
    for c in cases:
        heads.append(_Head(c, dev, heads[0].scratch if share_scratch and heads else None))
    rcs, snaps = [], []
    with options(unit_entry_dtype=kind_option(cases[0].kind)):
        for t0 in (t0s or [cases[0].t0]):
            arr = (_lib.HeadEx * max(len(heads), 1))(*[h.struct(t0) for h in heads])
            n = len(heads)
            if tweak is not None:
                n = tweak(arr, n) or n
            rcs.append(lib.bmi_head_fused_ex(arr, n, gh.stream()))
            torch.cuda.synchronize()
            snaps.append([h.snapshot() for h in heads])
    guards_ok = all(g.flanks_intact() for h in heads for g in h.guards())
    return rcs, snaps, guards_ok


def untouched(case, snap):
    """a launch that must write nothing left the prefill and the NaN logits."""
    init = acc_init(case)
    ok = all(snap[k] is None or torch.equal(snap[k], init[i]) for i, k in enumerate(("S1", "S2", "SL")))
    ok = ok and (snap["SH"] is None or torch.equal(snap["SH"], init[3, :, 0]))
    return ok and (snap["logits"] is None or bool(torch.isnan(snap["logits"]).all()))


# ---- the instantiation matrix (tests/test_head_exact.py, part (a)) -------------------------------------------------------------------
CS = (1, 10, 32, 33, 64, 65, 96, 100, 128)
ENTS = (False, True)
CALS = (None, "temp", "vec", "mat")
FORMS = ("single", "pack3")
KS = (32, 96, 288, 544, 1056)
HWS = (1, 4, 16, 12)
TCS = (1, 8, 31, 32, 33, 64, 70)
SITES = (None, "elem", "chan", "msk", "lsite")
BS = (2, 3, 5)


def _with_site(case, s):
    return replace(case, site=None if s == "lsite" else s, site_logits=s == "lsite")


def matrix_cases():
    """Every combination of class count, input kind, entropy, calibration state and launch form once: a list of (id, [HeadCase, ..]), one
    case per head of the launch.  K, HW, tc, the site and det / stochastic input rotate with the indices so that, for every class count and
    calibration state, every K, HW, tc and site value and both input forms occur (test_matrix_covers_every_value checks it).  The heads of
    a pack differ in K, HW, site, weights and det."""
    out = []
    for ic, C_ in enumerate(CS):
        for ik, kind in enumerate(KINDS):
            for ie, ent in enumerate(ENTS):
                for ical, cal in enumerate(CALS):
                    for iform, form in enumerate(FORMS):
                        j = ik * 4 + ie * 2 + iform
                        iK, iHW, isite = ik + ic, ie * 2 + iform + ic + ik, ik + ie + 2 * iform + ical
                        heads = []
                        for h in range(3 if form == "pack3" else 1):
                            c = HeadCase(C=C_, K=KS[(iK + h) % 5], HW=HWS[(iHW + h) % 4], B=BS[(ic + ik) % 3], tc=TCS[(j + ic + ical) % 7], t0=3,
                                         det=bool((ik + ie + ic + (h == 1)) % 2), kind=kind, cal=cal, ent=ent, seed=1 + h)
                            heads.append(_with_site(c, SITES[(isite + h) % 5]))
                        out.append((f"{form}-{heads[0].id}", heads))
    return out


def second_t0(case):
    """the first sample index of the second, accumulating launch."""
    return case.t0 + case.tc + 2


def _child(path):
    """python -m tests.exact_head OUT.npz: the class-tile counts 3 and 4 of the matrix for fp16 inputs, launched in THIS process (the test
    starts it with BMI_HEAD_CSPLIT=0: the K-split body) — every output of every head into one .npz."""
    out = {}
    for cid, heads in matrix_cases():
        if heads[0].rt < 3 or heads[0].kind != "f16":
            continue
        rcs, snaps, guards_ok = run_head(heads, t0s=[heads[0].t0, second_t0(heads[0])])
        out[f"{cid}|rc"] = np.array(rcs + [int(guards_ok)])
        for i, snap in enumerate(snaps):
            for h, s in enumerate(snap):
                for k, v in s.items():
                    if isinstance(v, torch.Tensor) and k != "gaps":
                        out[f"{cid}|{i}|{h}|{k}"] = v.numpy()
    np.savez(path, **out)


if __name__ == "__main__":
    import sys
    _child(sys.argv[1])
