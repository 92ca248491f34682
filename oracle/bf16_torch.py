"""ORACLE (test infrastructure): the bf16 matrix-core forward (GNN_FLAG_BF16_MLP) restated in the kernels' record
form, in torch on the CPU, rounded to bf16 at exactly the points where the kernels round.

`oracle/index_torch.py` is the reference's algebra; this module is the same algebra written the way
csrc/sell_pipeline.hip computes it on the bf16 route (hidden_dim 32 / 64, input_dim <= 8, n_iters > 0), so that a GPU
test can hold that route to the noise of fp32 accumulation instead of to the size of the bf16 effect.  With
rounding="none" it is the reference's forward (tests/test_oracle_bf16_host.py: index_torch at 1e-12).

Per-hit records of H = [h | X] (C = F + D columns; K = kTwoLog2e = 2 log2(e), the tanh -> exp2 scale):

    P = K (W1[:, :C] H + b1)    Q = K W1[:, C:] H       R = W3[:, :C] H    S = W3[:, C:2C] H    U = W3[:, 2C:] H + b3
    segment j = (s, d):  tanh(W1 [H_s | H_d] + b1) = 1 - 2 / (2^(P_s + Q_d) + 1)      (XP: 1 - 2 / (2^P_s 2^Q_d + 1))
                         e_j = sigmoid(W2 tanh(.) + b2)
    node sum of hit n:   U_n + sum_{d_j = n} e_j R_{s_j} + sum_{s_j = n} e_j S_{d_j};  h' = tanh(W4 tanh(sum) + b4)

What the kernels round (functions of sell_pipeline.hip), each point emulated below:

  rounding     fp32 -> bf16, round to nearest even: bf16_rne (integer form, k_pack16 and the X step) and pack_bf16
               (v_cvt_pk_bf16_f32, activations and records); here through fp32 first, as the device holds the
               value, then torch.bfloat16 (RNE; pinned to bf16_rne's formula by the host test)
  weights      k_pack16, once per forward: W4; the record rows of record_weight: P and Q rows = kTwoLog2e * W1
               scaled in fp32 THEN rounded (k_pack16's bf16_rne); R, S, U = the three C-wide blocks of W3, rounded
               there too.  Biases stay fp32 (k_pack16's last loops): b4, kTwoLog2e * b1, b3.
               Win / bin, W2 / b2 stay fp32 (k_pack's table: the input network and the score).
  H0           k_input4_bf: tanh(Win X + bin) in fp32 (role_gemv and tanh_f), rounded when used by the record
               product (act_frag inside mfma_records); X rounded in k_input4_bf's X step
  node hidden  q = tanh(sweep sum) (wide_hit_sweeps, called by k_iter_w and k_iter_wx; fp32, stored to the scratch),
               rounded as the W4 product's B operand (mfma_tail_scratch); hl = tanh(W4 q + b4) (mfma_tail_scratch)
               rounded as the record product's B operand (mfma_records' act_frag); X rounded again in
               mfma_tail_scratch's X step
  products     fp32 accumulation on v_mfma_f32_16x16x32_bf16 (mfma_tail_scratch, mfma_records), bias as the
               accumulator's start
  records      mfma_records: P, R, Q, S stored as bf16 (pack_bf16 after the exp2 in XP mode: P and Q are 2^x
               rounded, not 2^(rounded x)); U stays fp32; the LAST iteration's Pc / Qc stay fp32 and k_edge_w
               scores them with fp32 W2 / b2
  sweep        score_w: edge scores from the bf16 P / Q rows (the hit's own value through load_own_w is a bf16 row
               as well), fp32 arithmetic; node sums over the bf16 R / S rows (score_w's second loop) with fp32 e,
               starting from the fp32 U (wide_in_sweep, wide_hit_sweeps)
  NULL rows    k_pack16: P = bf16(kTwoLog2e b1), bf16(2^that) in XP mode; Q = 0, 1 in XP mode; R = S = 0.
               The sweeps read them only for the SELL padding past a list's end (sweep_w's index_of),
               where R = S = 0 makes the step add nothing: the node sums here run over the valid segments only.
               Padded segments (src = dst = -1) are scored by k_edge_w from the fp32 NULL rows of Pc / Qc
               (write_null_rows): P = kTwoLog2e b1 (2^that in XP mode), Q = 0 (1).
  route        choose_route: bf16 only for D in {32, 64}, F <= 8, n_iters > 0 and (Np + 2) D 4 < 2^32;
               n_iters = 0 declines it (the fp32 path runs)

Arguments of `segment_classifier`:
  rounding   "rne" (the kernels) or "none" (no rounding, K = 2 / ln 2 exactly: the reference's algebra)
  perturb    None or one named deviation from the kernels, for the discrimination test:
               "trunc"             every rounding point truncates instead of rounding to nearest even
               "x_unrounded"       X enters the products unrounded
               "q_unrounded"       the node hidden q enters the W4 product unrounded
               "records_fp32"      P, R, Q, S records kept fp32
               "scale_after_round" P / Q weights = kTwoLog2e * bf16(W1) instead of bf16(kTwoLog2e * W1)
               "exp2_after_round"  XP records 2^bf16(x) instead of bf16(2^x)
               "u_rounded"         U rounded to bf16
               "final_rounded"     the last iteration's Pc / Qc rounded to bf16
  accum      "fp64" (every product and sum in fp64 on the rounded operands: the reference for a GPU test) or
             "fp32" (the same in fp32, tanh in the kernels' form tanh_f: what fp32 arithmetic alone moves - values
             that land next to a bf16 rounding midpoint round the other way - the floor of a GPU bound)
  order      None or a permutation of the segments: the sums run in that order (scores come back in the caller's)
Thread count: torch's own (OMP_NUM_THREADS where it is set).
"""
import math

import numpy as np
import torch

K32 = torch.tensor(2.8853900817779268, dtype=torch.float32)       # kTwoLog2e (sell_pipeline.hip) in fp32
K64 = 2.0 / math.log(2.0)

PERTURBATIONS = ("trunc", "x_unrounded", "q_unrounded", "records_fp32", "scale_after_round", "exp2_after_round",
                 "u_rounded", "final_rounded")


def bf16_rne_bits(u):
    """sell_pipeline.hip bf16_rne, integer for integer, on uint32 bit patterns -> uint16: a NaN (exponent all ones,
    mantissa non-zero) keeps its upper half, sign included, with the quiet bit set; everything else is
    (u + 0x7FFF + ((u >> 16) & 1)) >> 16.  Without the NaN case the carry turns 0x7F800001 into +Inf (0x7F80),
    0x7FFFFFFF into -0.0 (0x8000) and 0xFFFFFFFF into +0.0.  torch.bfloat16 keeps a NaN a NaN as well but gives every
    one the same pattern: the two agree bit for bit on everything that is not a NaN, and on which inputs are."""
    u = np.asarray(u, np.uint32)
    rne = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), rne)


def bf16_round(v, mode="rne"):
    """v rounded to bf16 through fp32 (the value the device holds), returned in v's dtype.  mode: "rne" | "trunc"."""
    f = v.to(torch.float32)
    if mode == "rne":
        r = f.to(torch.bfloat16).to(torch.float32)
    elif mode == "trunc":
        r = (f.view(torch.int32) & -65536).view(torch.float32)
    else:
        raise ValueError(mode)
    return r.to(v.dtype)


def _weights(weights):
    from .dense_torch import KEYS
    if isinstance(weights, dict):
        weights = [weights[k] for k in KEYS]
    return [torch.as_tensor(w).detach().cpu() for w in weights]


def segment_classifier(X, src, dst, weights, n_iters, xp, rounding="rne", perturb=None, accum="fp64", order=None):
    """Edge scores [E] (float64) of the bf16 route for `weights` (the ten tensors the kernel receives, state_dict
    order or a dict by name: model.effective_weights(), or the compacted ones of a masked model at the width they
    run at).  `xp`: GNN_FLAG_EXP_PRODUCT (records 2^P, 2^Q)."""
    if rounding not in ("rne", "none") or (perturb is not None and perturb not in PERTURBATIONS):
        raise ValueError((rounding, perturb))
    if perturb is not None and rounding == "none":
        raise ValueError("a perturbation of the rounding needs rounding='rne'")
    if perturb == "exp2_after_round" and not xp:
        raise ValueError("exp2_after_round needs xp")
    dt = {"fp64": torch.float64, "fp32": torch.float32}[accum]
    exact = rounding == "none"
    Win, bin_, W1, b1, W2, b2, W3, b3, W4, b4 = _weights(weights)
    D, F = Win.shape
    C = F + D
    assert n_iters > 0 and W1.shape == (D, 2 * C) and W3.shape == (D, 3 * C)

    mode = "trunc" if perturb == "trunc" else "rne"

    def rnd(v, on=True):
        return v if exact or not on else bf16_round(v, mode)

    # weights (k_pack16): P / Q rows scaled in fp32, then rounded; R / S / U / W4 rounded; biases fp32
    if exact:
        Pw, Qw, bP = K64 * W1[:, :C].double(), K64 * W1[:, C:].double(), K64 * b1.double()
    elif perturb == "scale_after_round":
        Pw = K32 * rnd(W1[:, :C].float())
        Qw = K32 * rnd(W1[:, C:].float())
        bP = K32 * b1.float()
    else:
        Pw, Qw, bP = rnd(K32 * W1[:, :C].float()), rnd(K32 * W1[:, C:].float()), K32 * b1.float()
    Rw, Sw, Uw = rnd(W3[:, :C].float()), rnd(W3[:, C:2 * C].float()), rnd(W3[:, 2 * C:].float())
    W4r = rnd(W4.float())
    Wm = torch.cat([Pw, Rw, Qw, Sw, Uw]).to(dt).t().contiguous()          # [C, 5D]: one product for all records
    bm = torch.cat([bP.to(dt), torch.zeros(3 * D, dtype=dt), b3.to(dt)]).reshape(1, -1)
    W4t, b4 = W4r.to(dt).t().contiguous(), b4.to(dt)
    W2v, b2v = W2.to(dt).reshape(-1), b2.to(dt).reshape(())
    exp2 = torch.exp2
    if accum == "fp32":      # the kernels' tanh_f (common.h): 1 - 2 / (2^(K x) + 1), absolute (not relative) fp32 error
        def tanh(x):
            return 1.0 - 2.0 / (exp2(x * K32) + 1.0)
    else:
        tanh = torch.tanh

    X = torch.as_tensor(X).to(dt)
    N = X.shape[0]
    src = torch.as_tensor(src).long()
    dst = torch.as_tensor(dst).long()
    E = src.shape[0]
    perm = None
    if order is not None:
        perm = torch.as_tensor(order).long()
        src, dst = src[perm], dst[perm]
    valid = src >= 0
    vs, vd = src[valid], dst[valid]
    xb = X if perturb == "x_unrounded" else rnd(X)

    def records(h, last):
        """records of H = [h | X]: the five blocks [N, D] each (only P, Q when last), as the next pass reads them"""
        A = torch.cat([rnd(h), xb], 1) @ Wm + bm
        P, R, Q, S, U = A[:, :D], A[:, D:2 * D], A[:, 2 * D:3 * D], A[:, 3 * D:4 * D], A[:, 4 * D:]
        if last:                                         # Pc / Qc: fp32 rows (2^x in XP mode), scored by k_edge_w
            if xp:
                P, Q = exp2(P), exp2(Q)
            if perturb == "final_rounded":
                P, Q = rnd(P), rnd(Q)
            return P, Q
        rec = perturb != "records_fp32"
        if xp:
            if perturb == "exp2_after_round":
                P, Q = exp2(rnd(P)), exp2(rnd(Q))
            else:
                P, Q = rnd(exp2(P), rec), rnd(exp2(Q), rec)
        else:
            P, Q = rnd(P, rec), rnd(Q, rec)
        R, S = rnd(R, rec), rnd(S, rec)
        if perturb == "u_rounded":
            U = rnd(U)
        return P, R, Q, S, U

    def scores(P, Q, s, d):
        a = P[s] * Q[d] + 1.0 if xp else exp2(P[s] + Q[d]) + 1.0
        t = 1.0 - 2.0 / a                                # tanh of the edge network's hidden layer
        return torch.sigmoid(t @ W2v + b2v)

    # input network (fp32 on the device, rounded when the record product reads it)
    h = tanh(X @ Win.to(dt).t() + bin_.to(dt))
    P, R, Q, S, U = records(h, False)
    for t in range(n_iters):
        e = scores(P, Q, vs, vd)[:, None]
        acc = U.index_add(0, vd, e * R[vs]).index_add(0, vs, e * S[vd])
        q = tanh(acc)
        hl = tanh((q if perturb == "q_unrounded" else rnd(q)) @ W4t + b4)
        if t + 1 < n_iters:
            P, R, Q, S, U = records(hl, False)
        else:
            P, Q = records(hl, True)
    # final pass over every segment; padded ones read the fp32 NULL rows (write_null_rows)
    Pn = (K64 * b1.double() if exact else K32 * b1.float()).to(dt).reshape(1, D)
    Qn = torch.zeros(1, D, dtype=dt)
    if xp:
        Pn, Qn = exp2(Pn), Qn + 1.0
    Pt, Qt = torch.cat([P, Pn]), torch.cat([Q, Qn])
    e = scores(Pt, Qt, torch.where(valid, src, N), torch.where(valid, dst, N)).double()
    if perm is not None:
        out = torch.empty(E, dtype=torch.float64)
        out[perm] = e
        e = out
    return e
