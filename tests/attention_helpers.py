"""References, derived bounds, guarded buffers, padding poison, softmax regimes and case tables for the attention family: the forward
(csrc/attention.hip through lseg_op_attention_ex), its backward (csrc/attention_bwd2.hip through lseg_op_attention_backward_qkv) and the
split-precision forward (csrc/strict.hip through lseg_op_attention_strict).

Reference.  fp64 torch on the operands after their rounding to the operand type, written from the operation:
  forward    out = softmax(Q K^T scale [+ causal -inf mask]) V; pre-scaled: softmax2(Q' K^T) V; lse2 = log2 sum_k 2^(s_k scale log2 e)
  backward   what the kernel is specified to compute FROM ITS INPUTS (the given 16-bit o, the given fp32 lse2):
             P = exp2(S c - lse2), D = rowsum(dO o O), dS = P o (dO V^T - D) scale, dQ = dS K, dK = dS^T Q, dV = P^T dO
             (formula_equals_autograd shows it is fp64 autograd through softmax(Q K^T scale) V when o and lse2 are not rounded)
  strict     the forward on hi + lo of each plane.

Bound, derived (U24 = 2^-24 = one fp32 rounding, U23 = 2^-23 = one ulp, u_T = 2^-8 bf16 | 2^-11 fp16 = one rounding to the operand type,
tau_T = 2^-25 fp16 (half the subnormal spacing: fp16's absolute error below 2^-14) | 2^-126 bf16).  Scores in log2 units: s_k.
u_T is the unit roundoff of an 8-bit / 11-bit significand: just above a power of two the spacing is 2^-7 / 2^-10 of the value and round
to nearest moves it by half of that.  2^-9 / 2^-12 is the error at the TOP of a binade, not a bound: with it the fp32 emulation of the
plain kernel -- correct by construction -- lands at 1.27 of the bound (fwd2.bf16.pre0.N32.bh8.ramp), so it cannot be the worst case.
 1. exp2 argument.  A product of two 16-bit values is exact in fp32, the 64 additions of q.k round (64 U24 c A_k, A_k = sum_d |q_d||k_kd|),
    the fp32 constant scale*log2(e) is rounded (U24 |s_k|), the fused multiply-add that subtracts the running maximum rounds once
    (U24 |s_k - m|).  The pre-scaled kernel starts the accumulator at minus its reference maximum (partial sums up to A_k + M, M = max_k
    |s_k|), moves the reference with one rounded add per refresh (at most one per key tile, U24 M each) and subtracts the move from the
    scores (U24 |s_k - m|).  Both are inside  eps = U24 (64 c A_k + (68 + tiles) M).  v_exp_f32 is documented to 1 ulp:
    the probability before its rounding has the relative error  rho = ln2 eps + U23  (the row's largest A_k is used).
 2. P is rounded ONCE to the operand type: u_T relative, tau_T absolute in units of the row's largest probability (the kernels' running
    reference never exceeds the final maximum, so an absolute error made earlier only shrinks).  This is the dominant term.
 3. Normaliser.  The plain kernel divides by the sum of the UNROUNDED probabilities, so the roundings of 2. stay in the numerator alone:
    u_T W_d, W_d = sum_k P_k |v_kd|.  The pre-scaled kernel divides by the sum of the ROUNDED ones (lacc on the matrix pipe): numerator
    and normaliser carry the same factors and only the spread of v counts: u_T dev_d, dev_d = sum_k P_k |v_kd - out_d|, bounded here by
    min(W_d + |out_d|, weighted standard deviation of v_.d) -- far tighter wherever one key carries the row.  The errors of 1. are common
    to numerator and normaliser in both kernels (rho dev_d), and so is every rescale factor exp2(m_old - m_new).
 4. fp32 accumulation of P V and of the row sum: one rounding per key and per rescale: (keys + tiles + 4) U24 (W_d + |out_d|).
    The reciprocal of the row sum and the product with it: 3 U23 |out_d|.
 5. Second-order terms: the sum of 2. and 3. is multiplied by 1 + 4 u_T.
 6. The output is rounded once: 16-bit outputs are held to the INTERVAL [round_T(ref - b), round_T(ref + b)] as in tests/gemm_helpers.py.
 lse2 is checked in absolute terms: relative error r of the row sum (rho + (keys + tiles + 4) U24, pre-scaled: + u_T + tau_T keys / l)
 gives r (1 + r) / ln2; v_log_f32 at 1 ulp of a logarithm that can sit 8 above the true one: U23 (|log2 l| + 9); the reference's roundings
 and the final add: U24 ((tiles + 1) M + |lse2|).
 Backward, the same way: arg error eps = U24 (64 c A_ik + |s_ik| + |s_ik - L_i|), rho = ln2 eps + U23; D and dO.v accumulate in fp32
 (66 U24 sum|dO o O|, 65 U24 sum|dO||v|); dS' = P (dP - D) carries a_ik = P_ik ((rho_ik + 2 U24)|dP_ik - D_i| + e_dP + e_D) and one
 rounding to the operand type: g_ik = (a_ik + u_T |dS'_ik|)(1 + 4 u_T) + tau_T; P carries h_ik = P_ik (rho_ik + u_T)(1 + 4 u_T) + tau_T.
   dQ_id: scale (sum_k g_ik |k_kd| + (keys + 4) U24 sum_k |dS'_ik||k_kd|) + 2 U24 |dQ_id|; dK_kd alike over the queries with |q_id|;
   dV_kd: sum_i h_ik |dO_id| + (queries + 4) U24 sum_i P_ik |dO_id|; each output then rounded once (interval).
 Strict: fp32 throughout.  Score: 66 U24 scale A_ik; __expf = exp2(x log2 e): two roundings of an argument up to 2 M (4 U24 M) and 2 ulp;
 rho = U24 (66 scale A + 4 M) + 2 U23 (natural-log units); accumulation with one rescale per key: (keys + 24) U24 (W_d + |out_d|); the
 stored hi + lo pair: 2^-22 |out_d| + 2^-25.  The normaliser is the sum of the same fp32 probabilities: rho meets dev_d.

Guards: tests/gemm_helpers.Out.  Written cells are pre-filled with NaN and end finite; every other cell (lse2 rows >= Ntok, PRE, POST)
keeps its pattern bit for bit.  Padding poison: seeded finite non-zero values of the data's magnitude exactly where the contract in
include/lseg_hip.h allows them (forward: q, k, vt; backward: k, vt, and q with lse2 rows chosen so that the recomputed probability stays
<= 1); `poison=False` builds the zero-padded twin.

tests/test_attention_family_host.py feeds fp32 emulations and wrong variants through the same check functions;
tests/test_gpu_attention_family.py feeds the kernels' outputs.
"""
import ctypes as C
import math

import numpy as np
import torch

from gemm_helpers import LD, PRE, TD, Out, round_to  # noqa: F401  (PRE, LD re-exported to the tests)
from glue_helpers import RATIOS, _bits, assert_bits_equal, assert_within  # noqa: F401

U24, U23 = 2.0 ** -24, 2.0 ** -23
UT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TAU = {"bf16": 2.0 ** -126, "f16": 2.0 ** -25}
LOG2E, LN2 = 1.4426950408889634, math.log(2.0)
SHAPE = {3: (1, 3), 8: (2, 4), 512: (32, 16), 176: (11, 16), 171: (9, 19)}      # B * H -> (B, H)
SHARE = {}                    # case name -> share of 16-bit outputs whose interval has two distinct ends
THR_AMOUNTS = (7.5, 8.5, 0.0, -3.0)


def f32(x):
    return float(np.float32(x))


def npad_of(n):
    return (n + 127) // 128 * 128


def c2_of(c):
    """The kernels' fp32 constant scale * log2(e) (1 for the pre-scaled form, whose q carries it)."""
    return 1.0 if c.get("pre") else float(np.float32(c["scale"]) * np.float32(1.4426950408889634))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def case(name, kind, dt, BH, N, regime, nw=0, pre=0, causal=0, scale=0.125, poison=True, **kw):
    B, H = SHAPE[BH]
    return dict(name=name, kind=kind, dt=dt, B=B, H=H, BH=BH, N=N, npad=npad_of(N), regime=regime, nw=nw, pre=pre, causal=causal,
                scale=f32(scale), poison=poison, **kw)


NTOK_2W = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
OTHER = ("plain", "spike", "ramp", "low", "high", "flat", "thr")


def _fwd2_cases():
    """2-wave kernels (narrow grids): every Ntok meets `onehot` in every kernel; a second regime rotates, on the other B * H."""
    cs = []
    for dt in ("bf16", "f16"):
        for pre in (0, 1):
            for i, N in enumerate(NTOK_2W):
                bh = (3, 8)[(i + pre) % 2]
                cs.append(case(f"fwd2.{dt}.pre{pre}.N{N}.bh{bh}.onehot", "fwd", dt, bh, N, "onehot", nw=2, pre=pre))
                reg = OTHER[(i + 3 * pre + (dt == "f16")) % len(OTHER)]
                if reg == "thr" and N < 65:
                    reg = "plain"
                sc = 0.2 if (not pre and i % 3 == 0) else 0.125
                cs.append(case(f"fwd2.{dt}.pre{pre}.N{N}.bh{11 - bh}.{reg}" + (".s0.2" if sc == 0.2 else ""), "fwd", dt, 11 - bh, N, reg, nw=2,
                               pre=pre, scale=sc))
            for N in (129, 193):                # the refresh threshold from both sides inside one wave, with a stage reused
                nm = f"fwd2.{dt}.pre{pre}.N{N}.bh3.thr"
                if not any(c["name"] == nm for c in cs):
                    cs.append(case(nm, "fwd", dt, 3, N, "thr", nw=2, pre=pre))
            cs.append(case(f"fwd2.{dt}.pre{pre}.N33.bh3.low", "fwd", dt, 3, 33, "low", nw=2, pre=pre))
    return cs


def _fwd4_cases():
    """4-wave non-causal kernels: B * H = 512 at 65 and 128 tokens, 176 (head -> XCD map) and 171 (plain map) at 257 tokens, whose last
    query block has one live wave and three that only stream."""
    cs = []
    regs = ("plain", "onehot", "thr")
    for di, dt in enumerate(("bf16", "f16")):
        for pre in (0, 1):
            for si, (bh, N) in enumerate(((512, 65), (512, 128), (176, 257), (171, 257))):
                reg = regs[(si + pre + di) % 3]
                cs.append(case(f"fwd4.{dt}.pre{pre}.bh{bh}.N{N}.{reg}", "fwd", dt, bh, N, reg, nw=4, pre=pre))
            cs.append(case(f"fwd4.{dt}.pre{pre}.bh176.N257.onehot+", "fwd", dt, 176, 257, "onehot", nw=4, pre=pre))
    return cs


def _causal_cases():
    cs = []
    for dt in ("bf16", "f16"):
        for i, N in enumerate((1, 64, 65, 77, 128, 129, 200)):
            for bh in (3, 8):
                cs.append(case(f"causal.{dt}.N{N}.bh{bh}.onehot", "fwd", dt, bh, N, "onehot", nw=4, causal=1))
            bh = (3, 8)[i % 2]
            cs.append(case(f"causal.{dt}.N{N}.bh{bh}.spike", "fwd", dt, bh, N, "spike", nw=4, causal=1))
    return cs


def _bwd_cases():
    cs = []
    for di, dt in enumerate(("bf16", "f16")):
        for i, N in enumerate((1, 63, 64, 65, 127, 128, 129, 193, 257)):
            bh, sc = (3, 8)[(i + di) % 2], (0.125, 0.2)[i % 2]
            cs.append(case(f"bwd.{dt}.N{N}.bh{bh}.s{sc}.onehot", "bwd", dt, bh, N, "onehot", scale=sc))
            cs.append(case(f"bwd.{dt}.N{N}.bh{11 - bh}.s{0.325 - sc:.3g}.plain", "bwd", dt, 11 - bh, N, "plain", scale=0.325 - sc))
        cs.append(case(f"bwd.{dt}.N129.bh3.s0.125.plain.from-forward", "bwd", dt, 3, 129, "plain", from_forward=True))
    return cs


def _strict_cases():
    return [case(f"strict.N{N}.{reg}", "strict", "f16", 3, N, reg) for N in (1, 3, 4, 5, 63, 64, 65, 130) for reg in ("plain", "onehot", "low")]


FWD2, FWD4, CAUSAL, BWD, STRICT = _fwd2_cases(), _fwd4_cases(), _causal_cases(), _bwd_cases(), _strict_cases()
# the zero-padded twins of one forward and one backward case (bit-equal outputs)
TWIN_FWD = next(c for c in FWD2 if c["name"] == "fwd2.bf16.pre0.N65.bh3.onehot")
TWIN_BWD = next(c for c in BWD if c["name"] == "bwd.bf16.N65.bh8.s0.2.onehot")
ALL = FWD2 + FWD4 + CAUSAL + BWD + STRICT
assert len({c["name"] for c in ALL}) == len(ALL)
BY_NAME = {c["name"]: c for c in ALL}


def ids(cs):
    return [c["name"] for c in cs]


# ---- the launcher's plan -------------------------------------------------------------------------------------------------------------
def plan(lib, c, cus):
    out6 = (C.c_int * 6)()
    r = lib.lseg_op_attention_plan(c["B"], c["H"], c["N"], c["causal"], c["pre"], cus, C.byref(out6))
    return r, tuple(out6)


def expected_plan(c):
    nw, N = c["nw"], c["N"]
    nqb = -(-N // (32 * nw))
    return (nw, nqb, nqb * c["BH"], -(-N // 64), int(c["BH"] % 8 == 0), 32768)


# ---- softmax regimes (data builders) -------------------------------------------------------------------------------------------------
def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def designated_keys(N, causal):
    """The keys `onehot` cycles over (non-causal): key 0, key N - 1, the first and last key of every 64-key tile."""
    ks = [0, N - 1]
    for t in range(0, N, 64):
        ks += [t, min(t + 63, N - 1)]
    return ks


def onehot_targets(N, causal):
    ks = designated_keys(N, causal)
    tgt = []
    for i in range(N):
        if causal:
            opts = [i, max(i - 1, 0), 0, (i // 64) * 64, max((i // 64) * 64 - 1, 0)]       # the diagonal, just below it, tile edges at or below it
            tgt.append(opts[i % len(opts)])
        else:
            tgt.append(ks[i % len(ks)])
    return torch.tensor(tgt)


def regime_qk(c, seed):
    """-> (qs, k) fp32 [BH, N, 64]: qs is q in log2 units (qs . k is the exp2 argument before the maximum is subtracted)."""
    BH, N, reg = c["BH"], c["N"], c["regime"]
    base = 0.125 * LOG2E
    qs, k = _randn((BH, N, 64), seed) * base, _randn((BH, N, 64), seed + 1)
    if reg == "onehot":                    # q_i = 0.5 k_t: about 32 on the designated key, |.| < 14 elsewhere
        qs = 0.5 * k[:, onehot_targets(N, c["causal"])]
    elif reg == "spike":                   # one key dominates one query late in the sequence: the running maximum jumps
        k[:, max(N - 3, 0)] = qs[:, min(5, N - 1)] / base * 6.0
    elif reg == "ramp":                    # scores grow steadily along the keys: refresh after refresh
        qs[:, :, 0], k[:, :, 0] = 1.0, torch.linspace(0, 24, N).expand(BH, N)
    elif reg in ("low", "high"):           # every score near -200 / +200: 2^-200 underflows fp32
        qs[:, :, 0], k[:, :, 0] = 14.125, (-14.125 if reg == "low" else 14.125)
    elif reg == "flat":                    # identical keys: the output is the mean of V
        k = k[:, :1].expand(BH, N, 64).contiguous()
    elif reg == "thr":                     # tile 1 exceeds tile 0's row maximum by 7.5, 8.5, 0 or -3, rotating over the lanes of a wave
        assert N > 64
        qs, k = qs * 0.1, k * 0.3
        qs[:, :, 0], k[:, :, 0] = 1.0, 0.0
        qs[:, :, 1] = torch.tensor(THR_AMOUNTS)[torch.arange(N) % 4].expand(BH, N)
        k[:, :, 1] = ((torch.arange(N) >= 64) & (torch.arange(N) < 128)).float().expand(BH, N)
    else:
        assert reg == "plain", reg
    return qs, k


_DATA = {}


def _pad_rows(x, npad, fill):
    """[BH, N, 64] -> [BH, npad, 64] with the padded rows from `fill` (same dtype) or zero."""
    BH, N, _ = x.shape
    p = torch.zeros((BH, npad, 64), dtype=x.dtype) if fill is None else fill.clone()
    p[:, :N] = x
    return p


def data(c):
    """Seeded operands of a case, cached: q, k, v [BH, N, 64] in the operand type; qp, kp [BH, npad, 64], vtp [BH, 64, npad] padded
    (poisoned where the contract allows); backward: dO, o [B, N, H*64], lse2p [BH, npad] fp32; strict: hi / lo planes of each."""
    key = (c["kind"], c["dt"], c["BH"], c["N"], c["regime"], c["pre"], c["causal"], c["scale"], c["poison"])
    if key in _DATA:
        return _DATA[key]
    BH, N, npad, dt = c["BH"], c["N"], c["npad"], TD[c["dt"]]
    seed = 7000 + 13 * N + BH + 101 * OTHER.index(c["regime"]) if c["regime"] in OTHER else 9000 + 13 * N + BH
    qs, k32 = regime_qk(c, seed)
    v32 = _randn((BH, N, 64), seed + 2)
    d = {}
    if c["kind"] == "strict":              # fp32 values as (hi, lo) fp16 planes; the reference works on hi + lo
        q32 = qs / (c["scale"] * LOG2E)
        for nm, x in (("q", q32), ("k", k32), ("v", v32)):
            hi = x.to(torch.float16)
            lo = (x - hi.float()).to(torch.float16)
            d[nm + "_hi"], d[nm + "_lo"] = hi, lo
            d[nm] = hi.double() + lo.double()
        pl = lambda nm: torch.stack([_pad_rows(d[nm + "_hi"], npad, None), _pad_rows(d[nm + "_lo"], npad, None)])       # [2, BH, npad, 64]
        d["qp"], d["kp"] = pl("q"), pl("k")
        d["vtp"] = pl("v").transpose(-1, -2).contiguous()                                                                 # [2, BH, 64, npad]
        _DATA[key] = d
        return d
    q = (qs if c["pre"] else qs / (c["scale"] * LOG2E)).to(dt)           # ONE rounding, as the QKV epilogue does it
    k, v = k32.to(dt), v32.to(dt)
    poison = (lambda s: _randn((BH, npad, 64), seed + s).to(dt)) if c["poison"] else (lambda s: None)
    d.update(q=q, k=k, v=v, qp=_pad_rows(q, npad, poison(10)), kp=_pad_rows(k, npad, poison(11)),
             vtp=_pad_rows(v, npad, poison(12)).transpose(1, 2).contiguous())
    if c["kind"] == "bwd":
        B, H = c["B"], c["H"]
        dO = _randn((B, N, H * 64), seed + 3)
        dO[:, ::5] = 0.0                   # some dO rows all zero
        d["dO"] = dO.to(dt)
        f = forward_reference(dict(c, kind="fwd"), d)
        d["o"] = round_to(f["ref"], c["dt"]).to(dt)
        lse = torch.zeros((BH, npad), dtype=torch.float32)
        if c["poison"] and npad > N:       # padded rows: of a real row's magnitude, and >= the padded q row's largest score: P <= 1
            s2 = d["qp"][:, N:].double() @ k.double().transpose(1, 2) * c2_of(c)
            u = torch.rand((BH, npad - N), generator=torch.Generator().manual_seed(seed + 13)) * 4
            lse[:, N:] = (s2.amax(-1) + u).float()
        lse[:, :N] = f["lse"].float()
        d["lse2p"] = lse
    _DATA[key] = d
    return d


def heads_to_rows(x, c):
    """[BH, N, 64] -> [B, N, H*64] (the forward's output layout)."""
    B, H, N = c["B"], c["H"], c["N"]
    return x.reshape(B, H, N, 64).transpose(1, 2).reshape(B, N, H * 64)


def rows_to_heads(x, c):
    B, H, N = c["B"], c["H"], c["N"]
    return x.reshape(B, N, H, 64).transpose(1, 2).reshape(B * H, N, 64)


# ---- forward: reference and bound --------------------------------------------------------------------------------------------------
def forward_reference(c, d):
    """-> ref, bound [B, N, H*64]; lse, lse_bound [BH, N] (fp64)."""
    q, k, v = d["q"].double(), d["k"].double(), d["v"].double()
    N, dt, pre = c["N"], c["dt"], c["pre"]
    cexact = 1.0 if pre else c["scale"] * LOG2E
    s2 = q @ k.transpose(1, 2) * cexact
    A = (q.abs() @ k.abs().transpose(1, 2) * cexact)
    valid = torch.ones(N, N, dtype=torch.bool)
    if c["causal"]:
        valid = torch.ones(N, N, dtype=torch.bool).tril()
    s2 = s2.masked_fill(~valid, float("-inf"))
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    P = p / l
    ref = P @ v
    lse = (m + torch.log2(l)).squeeze(-1)
    tiles = -(-N // 64)
    Minf = s2.masked_fill(~valid, 0.0).abs().amax(-1, keepdim=True)
    Amax = A.masked_fill(~valid, 0.0).amax(-1, keepdim=True)
    rho = LN2 * U24 * (64 * Amax + (68 + tiles) * Minf) + U23                      # [BH, N, 1]
    nk = valid.sum(-1).double().view(1, N, 1)
    W = P @ v.abs()
    dev = torch.minimum(W + ref.abs(), (P @ (v * v) - ref * ref).clamp(min=0).sqrt())
    vsum = (valid.double() @ v.abs())                                              # sum of |v_kd| over the row's keys
    uT, tau = UT[dt], TAU[dt]
    first = uT * (dev if pre else W)
    b = (1 + 4 * uT) * (first + rho * dev + tau / l * (vsum + nk * ref.abs())) + U24 * (nk + tiles + 4) * (W + ref.abs()) + 3 * U23 * ref.abs()
    r = rho + (nk + tiles + 4) * U24
    if pre:
        r = r + uT + tau * nk / l
    lb = r * (1 + r) / LN2 + U23 * (torch.log2(l).abs() + 9) + U24 * ((tiles + 1) * Minf + lse.abs().unsqueeze(-1))
    return dict(ref=heads_to_rows(ref, c), bound=heads_to_rows(b, c), lse=lse, lse_bound=lb.squeeze(-1))


def cached(fn, c, d):
    """The reference of a case, computed once and kept beside its operands (every input of it is part of the data's cache key)."""
    key = "_" + fn.__name__
    if key not in d:
        d[key] = fn(c, d)
    return d[key]


def check_interval(pay, dt, ref, bound, name):
    """Every stored 16-bit value against [round_T(ref - b), round_T(ref + b)].  Prints and records the worst |err| / (b + the output's
    own rounding, u_T |ref| + tau_T) -- a figure for the records; the assertion is the interval."""
    pay = pay.double()
    lo, hi = round_to(ref - bound, dt), round_to(ref + bound, dt)
    SHARE[name] = (lo != hi).double().mean().item()
    bad = (pay < lo) | (pay > hi)
    ratio = ((pay - ref).abs() / (bound + UT[dt] * ref.abs() + TAU[dt])).max().item()
    RATIOS[name] = ratio
    print(f"attn-ratio {name}: worst |err| / (bound + output rounding) = {ratio:.4f}, two-ended intervals {100 * SHARE[name]:.2f} %")
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {pay.numel()} values outside [round(ref - b), round(ref + b)], first at {i}: got "
                             f"{pay[i].item()!r} for [{lo[i].item()!r}, {hi[i].item()!r}], ref {ref[i].item()!r}")


def make_forward_outs(c, device, with_lse=True):
    B, H, N, npad, BH = c["B"], c["H"], c["N"], c["npad"], c["BH"]
    outs = {"out": Out((B, N, H * 64), c["dt"], torch.ones((B, N, H * 64), dtype=torch.bool), device)}
    if with_lse:
        must = torch.zeros((BH, npad), dtype=torch.bool)
        must[:, :N] = True
        outs["lse2"] = Out((BH, npad), "f32", must, device)
    return outs


def check_forward(c, d, outs, who=""):
    f = cached(forward_reference, c, d)
    check_interval(outs["out"].check(f"{who}{c['name']}.out"), c["dt"], f["ref"], f["bound"], f"{who}{c['name']}.out")
    if "lse2" in outs:
        pay = outs["lse2"].check(f"{who}{c['name']}.lse2")
        assert_within(pay[:, :c["N"]], f["lse"], f["lse_bound"], f"{who}{c['name']}.lse2")


# ---- backward: reference and bound -------------------------------------------------------------------------------------------------
def backward_formula(q, k, v, o, dO, lse2, c_log2, scale):
    """The specified computation in fp64 on [BH, N, 64] operands and lse2 [BH, N]."""
    P = torch.exp2(q @ k.transpose(1, 2) * c_log2 - lse2.unsqueeze(-1))
    D = (dO * o).sum(-1, keepdim=True)
    dP = dO @ v.transpose(1, 2)
    dS = P * (dP - D) * scale
    return dS @ k, dS.transpose(1, 2) @ q, P.transpose(1, 2) @ dO, P, dS


def backward_reference(c, d):
    """-> ref, bound [B*N, 3*H*64] (fp64) from the case's q, k, v, o, dO, lse2 as the kernel receives them."""
    N, dt, scale = c["N"], c["dt"], c["scale"]
    q, k, v = d["q"].double(), d["k"].double(), d["v"].double()
    o, dO = rows_to_heads(d["o"].double(), c), rows_to_heads(d["dO"].double(), c)
    L = d["lse2p"][:, :N].double()
    cl = scale * LOG2E
    dQ, dK, dV, P, dS = backward_formula(q, k, v, o, dO, L, cl, scale)
    dSp = dS / scale
    s2 = q @ k.transpose(1, 2) * cl
    A = q.abs() @ k.abs().transpose(1, 2) * cl
    rho = LN2 * U24 * (64 * A + s2.abs() + (s2 - L.unsqueeze(-1)).abs()) + U23
    eD = 66 * U24 * (dO * o).abs().sum(-1, keepdim=True)
    edP = 65 * U24 * (dO.abs() @ v.abs().transpose(1, 2))
    D = (dO * o).sum(-1, keepdim=True)
    dP = dO @ v.transpose(1, 2)
    uT, tau = UT[dt], TAU[dt]
    a = P * ((rho + 2 * U24) * (dP - D).abs() + edP + eD)
    g = (a + uT * dSp.abs()) * (1 + 4 * uT) + tau
    h = P * (rho + uT) * (1 + 4 * uT) + tau
    bQ = scale * (g @ k.abs() + (N + 4) * U24 * (dSp.abs() @ k.abs())) + 2 * U24 * dQ.abs()
    bK = scale * (g.transpose(1, 2) @ q.abs() + (N + 4) * U24 * (dSp.abs().transpose(1, 2) @ q.abs())) + 2 * U24 * dK.abs()
    bV = h.transpose(1, 2) @ dO.abs() + (N + 4) * U24 * (P.transpose(1, 2) @ dO.abs())
    B = c["B"]
    cat = lambda x, y, z: torch.cat([heads_to_rows(t, c) for t in (x, y, z)], -1).reshape(B * N, -1)
    return dict(ref=cat(dQ, dK, dV), bound=cat(bQ, bK, bV))


def make_backward_outs(c, device, ws_bytes=0):
    B, H, N = c["B"], c["H"], c["N"]
    shape = (B * N, 3 * H * 64)
    outs = {"dqkv": Out(shape, c["dt"], torch.ones(shape, dtype=torch.bool), device)}
    if ws_bytes:
        assert ws_bytes % 4 == 0
        outs["ws"] = Out((ws_bytes // 4,), "f32", torch.zeros((ws_bytes // 4,), dtype=torch.bool), device)      # only its guards are looked at
    return outs


def check_ws_guards(ws, name):
    a, b = _bits(ws.flat), _bits(ws.before)
    assert torch.equal(a[:PRE], b[:PRE]) and torch.equal(a[-PRE:], b[-PRE:]), f"{name}: the backward wrote outside its workspace"
    assert not torch.equal(a[PRE:-PRE], b[PRE:-PRE]), f"{name}: the supplied workspace was not used"


def check_backward(c, d, outs, who=""):
    f = cached(backward_reference, c, d)
    H64 = c["H"] * 64
    pay_all = outs["dqkv"].check(f"{who}{c['name']}.dqkv")
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * H64, (i + 1) * H64)
        check_interval(pay_all[:, sl], c["dt"], f["ref"][:, sl], f["bound"][:, sl], f"{who}{c['name']}.{part}")
    if "ws" in outs:
        check_ws_guards(outs["ws"], f"{who}{c['name']}.ws")


def formula_equals_autograd(N=37, seed=5, scale=0.2):
    """max relative difference between backward_formula with UNROUNDED o and lse2 and fp64 autograd through softmax(Q K^T scale) V."""
    q, k, v, dO = (_randn((2, N, 64), seed + i).double() for i in range(4))
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = torch.softmax(qa @ ka.transpose(1, 2) * scale, -1) @ va
    out.backward(dO)
    lse2 = torch.logsumexp(q @ k.transpose(1, 2) * scale, -1) * LOG2E
    dQ, dK, dV, _, _ = backward_formula(q, k, v, out.detach(), dO, lse2, scale * LOG2E, scale)
    return max(((x - y.grad).abs().max() / y.grad.abs().max()).item() for x, y in ((dQ, qa), (dK, ka), (dV, va)))


# ---- strict: reference and bound ---------------------------------------------------------------------------------------------------
def strict_reference(c, d):
    q, k, v = d["q"], d["k"], d["v"]
    N, scale = c["N"], c["scale"]
    s = q @ k.transpose(1, 2) * scale
    A = q.abs() @ k.abs().transpose(1, 2) * scale
    P = torch.softmax(s, -1)
    ref = P @ v
    W = P @ v.abs()
    dev = torch.minimum(W + ref.abs(), (P @ (v * v) - ref * ref).clamp(min=0).sqrt())
    rho = U24 * (66 * A.amax(-1, keepdim=True) + 4 * s.abs().amax(-1, keepdim=True)) + 2 * U23
    b = rho * (1 + 4 * rho) * dev + (N + 24) * U24 * (W + ref.abs()) + 2.0 ** -22 * ref.abs() + 2.0 ** -25
    return dict(ref=heads_to_rows(ref, c), bound=heads_to_rows(b, c))


def make_strict_outs(c, device):
    shape = (2, c["B"], c["N"], c["H"] * 64)                      # hi plane, lo plane
    return {"out": Out(shape, "f16", torch.ones(shape, dtype=torch.bool), device)}


def check_strict(c, d, outs, who=""):
    f = cached(strict_reference, c, d)
    pay = outs["out"].check(f"{who}{c['name']}.planes").double()
    assert_within(pay[0] + pay[1], f["ref"], f["bound"], f"{who}{c['name']}.out")


def check_case(c, d, outs, who=""):
    {"fwd": check_forward, "bwd": check_backward, "strict": check_strict}[c["kind"]](c, d, outs, who)


# ---- fp32 emulations of the kernels' arithmetic (host self-check), with the wrong variants --------------------------------------------
def emulate_forward(c, d, wrong=None, with_lse=True):
    """Tile-wise online softmax over 64-key tiles in fp32 on the PADDED operands, P rounded to the operand type, each kernel's own row
    sum, the pre-scaled reference maximum with its 2^8 refresh decided per 32-row wave.  -> guarded CPU buffers."""
    N, npad, BH, dt, pre, causal = c["N"], c["npad"], c["BH"], TD[c["dt"]], c["pre"], c["causal"]
    nw = c["nw"] or 4
    c2 = torch.tensor(c2_of(c), dtype=torch.float32)
    R = min(-(-N // 32) * 32, npad)
    qf, kf, vf = d["qp"][:, :R].float(), d["kp"].float(), d["vtp"].transpose(1, 2).float()
    row = torch.arange(R).view(1, R, 1)
    walked = torch.full((1, R, 1), npad)                          # keys below this are walked: the masks below decide the rest
    if wrong == "kv-end-short":                                   # the last tile of each query block's key range is not walked
        kv_end = torch.minimum((row // (32 * nw) + 1) * 32 * nw, torch.tensor(N)) if causal else torch.full((1, R, 1), N)
        walked = (-(-kv_end // 64) - 1) * 64
    o = torch.zeros(BH, R, 64)
    l = torch.zeros(BH, R, 1)
    m_run = torch.zeros(BH, R, 1) if pre else torch.full((BH, R, 1), -1e30)
    lim = N - 1 if wrong == "drop-last-key" else (N + 1 if wrong == "key-ntok" else N)
    for t in range(-(-N // 64)):
        src = t - 2 if (wrong == "stage-early" and t >= 2) else t
        kt, vt = kf[:, 64 * src:64 * src + 64], vf[:, 64 * src:64 * src + 64]
        key = (64 * t + torch.arange(64)).view(1, 1, 64)
        ok = (key < lim) & (key < walked)
        if causal:
            ok = ok & ((key < row) if wrong == "causal-lt" else (key <= row))
        s = qf @ kt.transpose(1, 2)
        if pre:
            s = (s - m_run).masked_fill(~ok, float("-inf"))
            mx = s.amax(-1, keepdim=True)
            if t == 0 and wrong != "first-ref-0":
                delta = mx
            else:
                fire = (mx > 8.0).view(BH, R // 32, 32).any(-1, keepdim=True).expand(BH, R // 32, 32).reshape(BH, R, 1)
                delta = torch.where(fire, mx.clamp(min=0), torch.zeros_like(mx))
            alpha = torch.exp2(-delta)
            m_run = m_run + delta
            s = s - delta
            if t > 0:
                l = l * alpha
                if wrong != "refresh-l-not-o":
                    o = o * alpha
            p = torch.exp2(s)
            pt = p.to(dt).float()
            l = l + pt.sum(-1, keepdim=True)
        else:
            s = s.masked_fill(~ok, float("-inf"))
            mx = s.amax(-1, keepdim=True) * c2
            m_new = torch.maximum(m_run, mx)
            alpha = torch.exp2(m_run - m_new)
            m_run = m_new
            p = torch.exp2(s * c2 - m_new)
            l = l * alpha + p.sum(-1, keepdim=True)
            if wrong != "no-rescale":
                o = o * alpha
            pt = p.to(dt).float()
        o = o + pt @ vt
    res = (o * (1.0 / l))[:, :N]
    lse = (torch.log2(l) if wrong == "lse-no-max" else m_run + torch.log2(l)).squeeze(-1)
    if wrong == "heads-swapped":
        res, lse = res[torch.arange(BH) ^ 1], lse[torch.arange(BH) ^ 1]
    outs = make_forward_outs(c, "cpu", with_lse)
    outs["out"].payload()[:] = heads_to_rows(res, c).to(dt)
    if with_lse:
        rows = R if wrong == "lse-pad-rows" else N
        outs["lse2"].payload()[:, :rows] = lse[:, :rows]
    return outs


def emulate_backward(c, d, wrong=None):
    """fp32 with 16-bit P and dS, on the padded operands: the dQ side masks the padded keys of the last tile, the dK / dV side walks
    the padded query rows of the last tile unmasked with dO = 0 and D = 0."""
    N, dt, scale = c["N"], TD[c["dt"]], torch.tensor(c["scale"], dtype=torch.float32)
    c2 = torch.tensor(c2_of(c), dtype=torch.float32)
    T = -(-N // 64) * 64
    qf, kf, vf = d["qp"][:, :T].float(), d["kp"][:, :T].float(), d["vtp"].transpose(1, 2)[:, :T].float()
    BH = c["BH"]
    dO = torch.zeros(BH, T, 64)
    o = torch.zeros(BH, T, 64)
    dO[:, :N], o[:, :N] = rows_to_heads(d["dO"].float(), c), rows_to_heads(d["o"].float(), c)
    L = d["lse2p"][:, :T].unsqueeze(-1)
    D = ((dO * dO) if wrong == "D-from-dOdO" else (dO * o)).sum(-1, keepdim=True)
    P = torch.exp2(qf @ kf.transpose(1, 2) * c2 - L)                  # [BH, T queries, T keys]
    dP = dO @ vf.transpose(1, 2)
    Pq = P.clone()
    if wrong != "dq-no-tail-mask":
        Pq[:, :, N:] = 0.0
    dSq = (Pq * (dP - D)).to(dt).float()
    dQ = (dSq @ kf) * scale
    dSk = (P * (dP - D)).to(dt).float()
    dK = dSk.transpose(1, 2) @ qf
    if wrong != "dk-no-scale":
        dK = dK * scale
    dV = P.to(dt).float().transpose(1, 2) @ dO
    outs = make_backward_outs(c, "cpu")
    outs["dqkv"].payload()[:] = torch.cat([heads_to_rows(x[:, :N], c) for x in (dQ, dK, dV)], -1).reshape(c["B"] * N, -1).to(dt)
    return outs


def emulate_strict(c, d, wrong=None):
    """fp32 on hi + lo: four key partitions (keys p, p + 4, ...), merged by their maxima; an empty partition weighs nothing."""
    N, scale = c["N"], torch.tensor(c["scale"], dtype=torch.float32)
    q, k, v = (d[n + "_hi"].float() + d[n + "_lo"].float() for n in ("q", "k", "v"))
    s = (q * scale) @ k.transpose(1, 2)
    ms, ls, os_ = [], [], []
    for p in range(4):
        if p >= N:
            ms.append(torch.full(s.shape[:2] + (1,), 0.0 if wrong == "empty-partition" else float("-inf")))
            ls.append(torch.zeros(s.shape[:2] + (1,)))
            os_.append(torch.zeros(s.shape[:2] + (64,)))
            continue
        sp = s[:, :, p::4]
        m = sp.amax(-1, keepdim=True)
        e = torch.exp(sp - m)
        ms.append(m); ls.append(e.sum(-1, keepdim=True)); os_.append(e @ v[:, p::4])
    mm = torch.stack(ms).amax(0)
    w = [torch.where(m == float("-inf"), torch.zeros_like(m), torch.exp(m - mm)) for m in ms]
    lt = sum(wi * li for wi, li in zip(w, ls))
    val = heads_to_rows(sum(wi * oi for wi, oi in zip(w, os_)) / lt, c)
    hi = val.to(torch.float16)
    outs = make_strict_outs(c, "cpu")
    outs["out"].payload()[0], outs["out"].payload()[1] = hi, (val - hi.float()).to(torch.float16)
    return outs


def emulate(c, d, wrong=None):
    return {"fwd": emulate_forward, "bwd": emulate_backward, "strict": emulate_strict}[c["kind"]](c, d, wrong)
