"""The float64 statement of the FC block (nmrgnn/model.py:191-196) and of its backward, shared by test_gpu_fc_block.py;
tests/test_fc_block_ref_host.py checks it on the CPU.  NumPy only.

  forward   x_{l+1} = act(x_l W_l + b_l) + x_l  for l < L-1 (F -> F, residual);  g = act(x_{L-1} W_{L-1} + b_{L-1})  (F -> F/2)
  backward  a function of the TAPE it is handed (x_0 .. x_{L-1} and g, float32 values), as the kernels are: the activation
            output of a hidden layer is s_l = x_{l+1} - x_l, formed here in float64, and g for the last layer.
              D_{L-1} = dg;   P_l = D_l act'(s_l);   dW_l = x_l^T P_l;   db_l = sum_rows P_l
              D_{l-1} = D_l + P_l W_l^T  (hidden layer l),   D_{L-2} = P_{L-1} W_{L-1}^T;   dx = D_{-1}
            Magnitudes by the same recursion on absolute values: Dmag_{L-1} = |dg|, Pmag_l = Dmag_l |act'|,
            Dmag_{l-1} = Dmag_l + Pmag_l |W_l|^T, mag(dW_l) = |x_l|^T Pmag_l, mag(db_l) = sum Pmag_l.

Criteria (the functions of tests/mp_layer_ref.py): per element |got - ref| <= c * mag + 1e-7 * max(mag) (check), and the statistic
r = rms(got - ref) / rms(mag) (rstat) held against sqrt(r32 * r_drop):
  r32     the statistic of a plain float32 numpy evaluation of the same formula
  r_drop  the statistic of the float64 evaluation with one `lo x hi` piece product missing:
            y_l, g   the activation operand x_l reduced to its leading fp16 piece under the fixed factor 2^4 (fc_fused.hip: FC_XS)
            dx       dP_l reduced to its leading piece under the row's own power-of-two scale in every dP_l W_l^T
            dW_l     x_l reduced to its leading fp16 piece in x_l^T dP_l
Both come from the reference side alone; no GPU result enters a threshold."""
import numpy as np

from mp_layer_ref import ACT, C_REL, STAT_MIN, act_fwd, act_grad_from_out, check, f32, lead_piece, rstat  # noqa: F401

FC_XS = 16.0                    # fc_fused.hip: activations enter the piece planes times 2^4
FC_XMAX = 65504.0 / FC_XS       # a tile with |x| at or beyond this is redone by the fp32 layers


# ---------------------------------------------------------------------------------------------------------- float64
def ref_layer_fwd(x, W, b, act, last):
    """one layer: (value, mag); the last layer has no residual"""
    s = act_fwd(act, x @ W + b)
    mag = np.abs(x) @ np.abs(W) + np.abs(b)
    return (s, mag) if last else (s + x, mag + np.abs(x))


def ref_fwd(x, Ws, bs, act):
    """the chain: (xs = [x_0 .. x_{L-1}], g, mags = [mag(x_1) .. mag(x_{L-1}), mag(g)])"""
    xs, mags = [x], []
    L = len(Ws)
    for l in range(L):
        v, m = ref_layer_fwd(xs[-1], Ws[l], bs[l], act, l == L - 1)
        xs.append(v)
        mags.append(m)
    return xs[:-1], xs[-1], mags


def ref_bwd(tape, g, Ws, dg, act):
    """(dx, dWs, dbs) and (mag dx, mag dWs, mag dbs) from the tape (float32 values held as float64)"""
    L = len(Ws)
    dWs, dbs, mWs, mbs = [None] * L, [None] * L, [None] * L, [None] * L
    D, Dm = dg, np.abs(dg)
    for l in range(L - 1, -1, -1):
        last = l == L - 1
        slope = act_grad_from_out(act, g if last else tape[l + 1] - tape[l])
        P, Pm = D * slope, Dm * np.abs(slope)
        dWs[l], dbs[l] = tape[l].T @ P, P.sum(0)
        mWs[l], mbs[l] = np.abs(tape[l]).T @ Pm, Pm.sum(0)
        back, backm = P @ Ws[l].T, Pm @ np.abs(Ws[l]).T
        D, Dm = (back, backm) if last else (D + back, Dm + backm)
    return (D, dWs, dbs), (Dm, mWs, mbs)


# ---------------------------------------------------------------------------------------------------------- statistic
def fixed_piece(x):
    """x reduced to the leading fp16 piece of 2^4 x (the forward's activation operand without its small piece)"""
    with np.errstate(over="ignore"):
        return (x * FC_XS).astype(np.float16).astype(np.float64) / FC_XS


def plain_piece(x):
    """x reduced to its leading fp16 piece, unscaled (the x operand of the dW product)"""
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(np.float64)


def fwd_stats(tape, Ws, bs, act):
    """[(r32, r_drop)] per layer, each layer on its own: layer l applied to tape[l] (float32 values)"""
    L = len(Ws)
    out = []
    t = np.float32
    for l in range(L):
        last = l == L - 1
        x = tape[l]
        v, m = ref_layer_fwd(x, Ws[l], bs[l], act, last)
        x32 = x.astype(t)
        s32 = act_fwd(act, x32 @ Ws[l].astype(t) + bs[l].astype(t)).astype(t)
        v32 = s32 if last else s32 + x32
        assert v32.dtype == t
        sd = act_fwd(act, fixed_piece(x) @ Ws[l] + bs[l])
        vd = sd if last else sd + x
        out.append((rstat(v32, v, m), rstat(vd, v, m)))
    return out


def bwd_stats(tape, g, Ws, dg, act, ref=None):
    """{"dx": (r32, r_drop), "dW": [(r32, r_drop)] * L} against ref_bwd of the same tape"""
    L = len(Ws)
    (dx, dWs, _), (mx, mWs, _) = ref if ref is not None else ref_bwd(tape, g, Ws, dg, act)
    slopes = [act_grad_from_out(act, g if l == L - 1 else tape[l + 1] - tape[l]) for l in range(L)]
    # ---- plain float32
    t = np.float32
    D = dg.astype(t)
    dW32 = [None] * L
    for l in range(L - 1, -1, -1):
        P = D * slopes[l].astype(t)
        dW32[l] = tape[l].astype(t).T @ P
        back = P @ Ws[l].astype(t).T
        D = back if l == L - 1 else D + back
    assert D.dtype == t and all(w.dtype == t for w in dW32)
    dx32 = D
    # ---- float64 with the small piece of one operand missing
    D = dg
    dWd = [None] * L
    for l in range(L - 1, -1, -1):
        P = D * slopes[l]
        dWd[l] = plain_piece(tape[l]).T @ P
        back = lead_piece(P) @ Ws[l].T
        D = back if l == L - 1 else D + back
    return {"dx": (rstat(dx32, dx, mx), rstat(D, dx, mx)),
            "dW": [(rstat(dW32[l], dWs[l], mWs[l]), rstat(dWd[l], dWs[l], mWs[l])) for l in range(L)]}


# ---------------------------------------------------------------------------------------------------------- data
def normal_data(rng, N, F, L, s=None):
    """random normal data, weights scaled so that pre-activations stay O(1); every array holds float32 values"""
    s = 0.8 / np.sqrt(F) if s is None else s
    Fh = F // 2
    x = f32(rng.standard_normal((N, F)))
    Ws = [f32(rng.standard_normal((F, F)) * s) for _ in range(L - 1)] + [f32(rng.standard_normal((F, Fh)) * s)]
    bs = [f32(rng.standard_normal(F) * 0.1) for _ in range(L - 1)] + [f32(rng.standard_normal(Fh) * 0.1)]
    dg = f32(rng.standard_normal((N, Fh)))
    return x, Ws, bs, dg


def exact_data(rng, N, F, L, nnz=4, dg_rows=256):
    """x0 in {-2..2}, W_l with about `nnz` non-zeros per column from {-1, +1}, b in {-1, 0, 1}, dg in {-2..2} on `dg_rows` randomly
    chosen rows and zero elsewhere"""
    Fh = F // 2
    x = rng.integers(-2, 3, (N, F)).astype(np.float64)
    Ws = [np.where(rng.random((F, n)) < nnz / F, rng.choice([-1.0, 1.0], (F, n)), 0.0) for n in [F] * (L - 1) + [Fh]]
    bs = [rng.integers(-1, 2, n).astype(np.float64) for n in [F] * (L - 1) + [Fh]]
    dg = np.zeros((N, Fh))
    if N:
        rows = rng.choice(N, min(dg_rows, N), replace=False)
        dg[rows] = rng.integers(-2, 3, (len(rows), Fh))
    return x, Ws, bs, dg


def sig_bits(a):
    """the largest number of significant bits of an entry of the integer-valued array a"""
    a = np.abs(np.asarray(a, np.float64))
    assert np.array_equal(a, np.floor(a)) and (a.size == 0 or a.max() < 2.0 ** 52)
    v = a[a > 0].astype(np.int64)
    if v.size == 0:
        return 0
    v = v // (v & -v)
    return int(np.floor(np.log2(v.max()))) + 1


def exact_conditions(x, Ws, bs, dg, act):
    """The conditions under which every branch must reproduce float64 bit for bit, asserted on the CPU; returns the float64
    results (xs, g, dx, dWs, dbs).  (1) the sum of absolute values of every output's terms stays below 2^24; (2) max |x_l| <
    FC_XMAX, so the piece body is not repaired away; (3) every operand (x_l, W_l, dP_l, D_l) has at most 11 significant bits,
    so one fp16 piece holds it."""
    L = len(Ws)
    xs, g, mags = ref_fwd(x, Ws, bs, act)
    tape = xs                                           # integers: the float32 tape is the float64 chain
    (dx, dWs, dbs), (mx, mWs, mbs) = ref_bwd(tape, g, Ws, dg, act)
    top = max([float(m.max()) if m.size else 0.0 for m in mags + [mx] + mWs + mbs])
    assert top < 2.0 ** 24, f"exact family: an abs-sum of {top} reaches 2^24"
    assert max(float(np.abs(v).max()) if v.size else 0.0 for v in xs) < FC_XMAX - 1, "exact family: a tile would be repaired"
    ops = list(xs) + list(Ws)
    D = dg
    for l in range(L - 1, -1, -1):
        last = l == L - 1
        P = D * act_grad_from_out(act, g if last else tape[l + 1] - tape[l])
        ops += [P, D]
        assert (float(np.abs(P).max()) if P.size else 0.0) < 2.0 ** 14
        back = P @ Ws[l].T
        D = back if last else D + back
    ops.append(D)
    for o in ops:                                       # (integers below 2^11 need no closer look)
        if o.size and np.abs(o).max() >= 2048.0:
            assert sig_bits(o) <= 11, f"exact family: an operand with {sig_bits(o)} significant bits"
    for v in [g, dx] + xs + dWs + dbs:
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return xs, g, dx, dWs, dbs
