"""Float64 reference of the GRU / LSTM recurrences behind include/morgana_hip.h (K3), with a DERIVED fp32 rounding bound per element.

Plain numpy, one loop per step, no GPU and no torch.  Gate order and formulas are those of torch.nn.GRU (r, z, n) and torch.nn.LSTM
(i, f, g, o):

    GRU   r = s(x_r + W_hr h + b_hr)   z = s(x_z + W_hz h + b_hz)   hn = W_hn h + b_hn   n = tanh(x_n + r hn)   h' = (1 - z) n + z h
    LSTM  i, f, o = s(x + W h + b)     g = tanh(x_g + W_hg h + b_hg)   c' = f c + i g   h' = o tanh(c')

Two layers of code:

* ``gru_run`` / ``lstm_run`` (+ ``_bwd``): the free-running recurrence over T with the length mask of the header's contract (state
  frozen, ``out`` zero, gate gradients zero past ``seq_len[b]``), in any dtype (float64 = the reference, float32 = an honest fp32
  evaluation whose distance from the reference calibrates the free-running test) and with an ``operand_round`` hook (``bf16_round``
  models the bf16-operand kernels: the state / gate-gradient operand and W_hh are rounded before the product, nothing else is).
* ``gru_step`` / ``lstm_step`` (+ ``_bwd``, ``state_grad``): ONE step in float64 from given operands, returning every quantity as a
  ``Bounded`` (value, bound) pair.

The bound is a property of fp32 arithmetic, not of any kernel.  A pre-activation p = x + sum_k a_k w_k + b evaluated in fp32 in ANY
summation order satisfies |p^ - p| <= gamma (|x| + sum_k |a_k| |w_k| + |b|), gamma = (K + 4) 2^-24.  Through the cell it is propagated
by first-order interval rules with 2^-23 of the magnitudes involved added per elementwise operation (``Bounded.__add__`` etc.), the
derivatives' maxima for the non-linearities (s' <= 1/4, tanh' <= 1), three operations' worth for an exp-based sigmoid / tanh, and, for the
``fast`` cell (gru_cell.h: v_exp_f32 + v_rcp_f32), the header's own absolute figure per sigmoid (FAST_SIGMOID_ABS, twice that for the
tanh form 2 s(2x) - 1).  Gradients of saturated gates reach the fp32 subnormals, where a product is rounded to a grid of spacing ETA =
2^-149 instead of relatively: every product adds ETA (a K-term dot product K ETA)."""
import numpy as np

F64 = np.float64
U = 2.0 ** -24            # unit roundoff of fp32
EPS = 2.0 ** -23          # charged per elementwise fp32 operation, times the magnitudes involved
ETA = 2.0 ** -149         # spacing of the fp32 subnormals: a product that underflows is off by up to this much in ABSOLUTE terms (the
                          # relative model (1 + d) holds for normal results only; sums and differences are exact down there)
FAST_SIGMOID_ABS = 2e-7   # csrc/gru_cell.h: absolute error of mg_sigmoid_fast


def gamma(k):
    """Forward error factor of a K-term fp32 sum of products plus the input projection and the bias, in any order."""
    return (k + 4) * U


# ------------------------------------------------------------------------------------------------------------ bf16 operand rounding
def bf16_bits(x):
    """float32 -> bf16 bit pattern (uint16), round to nearest even on the float32 bit pattern; NaN -> the quiet NaN 0x7FC0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32)
    rounded = ((bits + (np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), rounded)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(x):
    """x rounded to bf16, returned in x's floating dtype (every bf16 value is exact in float32 and float64)."""
    x = np.asarray(x)
    return bf16_to_f32(bf16_bits(x.astype(np.float32))).astype(x.dtype if x.dtype.kind == 'f' else np.float32)


# ------------------------------------------------------------------------------------------------------------ value +- bound
class Bounded:
    """A float64 value with a bound on |fp32 evaluation - value|; arithmetic adds EPS of the magnitudes per operation."""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=F64)
        self.e = np.broadcast_to(np.asarray(e, dtype=F64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Bounded) else Bounded(x)

    def __add__(self, o):
        o = Bounded.lift(o)
        return Bounded(self.v + o.v, self.e + o.e + EPS * (np.abs(self.v) + np.abs(o.v)))

    __radd__ = __add__

    def __sub__(self, o):
        o = Bounded.lift(o)
        return Bounded(self.v - o.v, self.e + o.e + EPS * (np.abs(self.v) + np.abs(o.v)))

    def __rsub__(self, o):
        return Bounded.lift(o) - self

    def __mul__(self, o):
        o = Bounded.lift(o)
        v = self.v * o.v
        return Bounded(v, self.e * np.abs(o.v) + np.abs(self.v) * o.e + self.e * o.e + EPS * np.abs(v) + ETA)

    __rmul__ = __mul__


def _sigmoid64(p):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-p))


def b_sigmoid(p, fast=False):
    v = _sigmoid64(p.v)
    return Bounded(v, 0.25 * p.e + 3 * EPS * v + (FAST_SIGMOID_ABS if fast else 0.0))


def b_tanh(p, fast=False):
    v = np.tanh(p.v)
    return Bounded(v, p.e + 3 * EPS * np.abs(v) + (2 * FAST_SIGMOID_ABS if fast else 0.0))


def _product(a, w, k=None):
    """a [B,K] x w [N,K]^T in float64 -> (value [B,N], sum_k |a||w|)."""
    a, w = np.asarray(a, dtype=F64), np.asarray(w, dtype=F64)
    return a @ w.T, np.abs(a) @ np.abs(w).T


def _preact(x, x_mag, prod, mag, bias, k):
    """x + prod + bias with the gamma bound.  x_mag: the magnitude sum behind x when x is itself an in-step projection (else |x|)."""
    v = x + prod + bias
    return Bounded(v, gamma(k) * (x_mag + mag + np.abs(bias)) + k * ETA)


# ------------------------------------------------------------------------------------------------------------ GRU, one step
def gru_step(xproj_t, h_prev_operand, h_prev, w_hh, b_hh, fast=False, xproj_mag=None):
    """One GRU step in float64.  xproj_t [B,3H]; h_prev_operand [B,H] enters the product (the fp32 state, or its bf16 shadow); h_prev [B,H]
    enters the blend; w_hh [3H,H] (the operand the kernel had: W_hh, or bf16(W_hh)); b_hh [3H].
    xproj_mag: for a stacked layer whose input projection is formed inside the step, sum |a||w| + |b| of that projection (K becomes 2H).
    Returns a dict of Bounded: r, z, n, hn (= W_hn h + b_hn), h_new."""
    x = np.asarray(xproj_t, dtype=F64)
    b = np.asarray(b_hh, dtype=F64)
    hprev = np.asarray(h_prev, dtype=F64)
    h = hprev.shape[1]
    k = h if xproj_mag is None else 2 * h
    xm = np.abs(x) if xproj_mag is None else np.asarray(xproj_mag, dtype=F64)
    prod, mag = _product(h_prev_operand, w_hh)
    sl = [slice(g * h, (g + 1) * h) for g in range(3)]
    r = b_sigmoid(_preact(x[:, sl[0]], xm[:, sl[0]], prod[:, sl[0]], mag[:, sl[0]], b[sl[0]], k), fast)
    z = b_sigmoid(_preact(x[:, sl[1]], xm[:, sl[1]], prod[:, sl[1]], mag[:, sl[1]], b[sl[1]], k), fast)
    hn = _preact(0.0, 0.0, prod[:, sl[2]], mag[:, sl[2]], b[sl[2]], h)
    xn = Bounded(x[:, sl[2]], 0.0 if xproj_mag is None else gamma(h) * xm[:, sl[2]])
    n = b_tanh(xn + r * hn, fast)
    h_new = (1.0 - z) * n + z * hprev
    return {'r': r, 'z': z, 'n': n, 'hn': hn, 'h_new': h_new}


def state_grad(gates_operand_next, w, carry, k=None):
    """d loss / d state from the later steps: carry + gates_operand_next [B,G] @ w [G,H] (G = 3H / 4H), as a Bounded.
    carry: Bounded or array [B,H]; gates_operand_next None = no later step (the value is the carry itself)."""
    carry = Bounded.lift(carry)
    if gates_operand_next is None:
        return carry
    a, w = np.asarray(gates_operand_next, dtype=F64), np.asarray(w, dtype=F64)
    prod, mag = a @ w, np.abs(a) @ np.abs(w)
    kk = a.shape[1] if k is None else k
    return Bounded(carry.v + prod, carry.e + gamma(kk) * (np.abs(carry.v) + mag) + kk * ETA)


def gru_step_bwd(dstate, grad_out_t, r, z, n, hn, h_prev, active=None):
    """Gradient of one GRU step.  dstate: Bounded / array [B,H] (d loss / d h_t from the later steps); grad_out_t [B,H] (array or Bounded);
    r, z, n, hn: the saved gates; h_prev = hstate[:, t]; active [B] bool (None = all).
    Returns Bounded dr, dz, dn, dnr (dxproj_t = dr|dz|dn, dhproj_t = dr|dz|dnr) and carry (elementwise part of d loss / d h_{t-1})."""
    dstate = Bounded.lift(dstate)
    r, z, n, hn, hp = (np.asarray(a, dtype=F64) for a in (r, z, n, hn, h_prev))
    dh = dstate + grad_out_t
    dn = dh * (1.0 - Bounded(z)) * (1.0 - Bounded(n) * n)
    dz = dh * (Bounded(hp) - n) * z * (1.0 - Bounded(z))
    dr = dn * hn * r * (1.0 - Bounded(r))
    dnr = dn * r
    carry = dh * z
    res = {'dr': dr, 'dz': dz, 'dn': dn, 'dnr': dnr, 'carry': carry}
    if active is not None:
        act = np.asarray(active, dtype=bool)[:, None]
        for key in ('dr', 'dz', 'dn', 'dnr'):
            res[key] = Bounded(np.where(act, res[key].v, 0.0), np.where(act, res[key].e, 0.0))
        res['carry'] = Bounded(np.where(act, carry.v, dstate.v), np.where(act, carry.e, dstate.e))
    return res


# ------------------------------------------------------------------------------------------------------------ LSTM, one step
def lstm_step(xproj_t, h_prev_operand, c_prev, w_hh, b_hh, fast=False, xproj_mag=None):
    """One LSTM step in float64 (arguments as gru_step; xproj_t [B,4H], w_hh [4H,H]).  Returns Bounded i, f, g, o, c_new, h_new."""
    x = np.asarray(xproj_t, dtype=F64)
    b = np.asarray(b_hh, dtype=F64)
    cprev = np.asarray(c_prev, dtype=F64)
    h = cprev.shape[1]
    k = h if xproj_mag is None else 2 * h
    xm = np.abs(x) if xproj_mag is None else np.asarray(xproj_mag, dtype=F64)
    prod, mag = _product(h_prev_operand, w_hh)
    pre = []
    for g in range(4):
        s = slice(g * h, (g + 1) * h)
        pre.append(_preact(x[:, s], xm[:, s], prod[:, s], mag[:, s], b[s], k))
    i, f, o = b_sigmoid(pre[0], fast), b_sigmoid(pre[1], fast), b_sigmoid(pre[3], fast)
    g = b_tanh(pre[2], fast)
    c_new = f * cprev + i * g
    h_new = o * b_tanh(c_new, fast)
    return {'i': i, 'f': f, 'g': g, 'o': o, 'c_new': c_new, 'h_new': h_new}


def lstm_step_bwd(dh_state, dc_state, grad_out_t, i, f, g, o, c_prev, c_new, active=None, fast=False):
    """Gradient of one LSTM step.  dh_state / dc_state: Bounded / array [B,H]; the saved gates and cell states of the step.
    Returns Bounded di, df, dg, do (dgates_t), carry_c (elementwise part of d loss / d c_{t-1}) and carry_h (0 on an active step: all of
    d loss / d h_{t-1} goes through the product with these gate gradients; the incoming dh_state on a padded one)."""
    dh_state, dc_state = Bounded.lift(dh_state), Bounded.lift(dc_state)
    i, f, g, o, cp, cn = (np.asarray(a, dtype=F64) for a in (i, f, g, o, c_prev, c_new))
    dh = dh_state + grad_out_t
    tc = b_tanh(Bounded(cn), fast)              # fast: the kernels that re-form tanh(c_t) as 2 s(2 c) - 1 (lstm_persist.hip)
    dc = dc_state + dh * o * (1.0 - tc * tc)
    res = {'di': dc * g * i * (1.0 - Bounded(i)), 'df': dc * cp * f * (1.0 - Bounded(f)), 'dg': dc * i * (1.0 - Bounded(g) * g),
           'do': dh * tc * o * (1.0 - Bounded(o)), 'carry_c': dc * f, 'carry_h': Bounded(np.zeros_like(cp))}
    if active is not None:
        act = np.asarray(active, dtype=bool)[:, None]
        for key in ('di', 'df', 'dg', 'do'):
            res[key] = Bounded(np.where(act, res[key].v, 0.0), np.where(act, res[key].e, 0.0))
        res['carry_c'] = Bounded(np.where(act, res['carry_c'].v, dc_state.v), np.where(act, res['carry_c'].e, dc_state.e))
        res['carry_h'] = Bounded(np.where(act, 0.0, dh_state.v), np.where(act, 0.0, dh_state.e))
    return res


def in_step_projection(below_operand, w_ih, b_ih):
    """The input projection a stacked layer forms inside its step: (value, magnitude sum) of below_operand [B,I] @ w_ih [G,I]^T + b_ih."""
    prod, mag = _product(below_operand, w_ih)
    b = np.asarray(b_ih, dtype=F64)
    return prod + b, mag + np.abs(b)


def handed_down_gradient(gates_operand, w_ih_above):
    """d out^l_t = gate gradients of the layer above [B,G] @ its W_ih [G,H], as a Bounded (K = G)."""
    return state_grad(gates_operand, w_ih_above, np.zeros((np.asarray(gates_operand).shape[0], np.asarray(w_ih_above).shape[1])))


# ------------------------------------------------------------------------------------------------------------ free-running recurrences
def _active(seq_len, t, b):
    return np.ones(b, dtype=bool) if seq_len is None else (t < np.asarray(seq_len))


def _sig(x):
    with np.errstate(over='ignore'):
        return (1 / (1 + np.exp(-x))).astype(x.dtype)


def _ident(x):
    return x


def gru_run(xproj, w_hh, b_hh, seq_len=None, h0=None, operand_round=None, dtype=F64):
    """xproj [B,T,3H].  Returns out [B,T,H], hstate [B,T+1,H], saved [B,T,4H] = (r, z, n, hn); saved past an item's length holds what the
    frozen state produces (UNSPECIFIED by the header: do not compare)."""
    rnd = operand_round or _ident
    x, w, bias = (np.asarray(a).astype(dtype) for a in (xproj, w_hh, b_hh))
    b, t, h3 = x.shape
    h = h3 // 3
    w_op = rnd(w)
    hstate = np.zeros((b, t + 1, h), dtype=dtype)
    if h0 is not None:
        hstate[:, 0] = np.asarray(h0).reshape(b, h)
    out = np.zeros((b, t, h), dtype=dtype)
    saved = np.zeros((b, t, 4 * h), dtype=dtype)
    one = dtype(1)
    for s in range(t):
        hp = hstate[:, s]
        hproj = rnd(hp) @ w_op.T + bias
        r = _sig(x[:, s, :h] + hproj[:, :h])
        z = _sig(x[:, s, h:2 * h] + hproj[:, h:2 * h])
        hn = hproj[:, 2 * h:]
        n = np.tanh(x[:, s, 2 * h:] + r * hn)
        hnew = (one - z) * n + z * hp
        act = _active(seq_len, s, b)[:, None]
        hstate[:, s + 1] = np.where(act, hnew, hp)
        out[:, s] = np.where(act, hnew, 0)
        saved[:, s] = np.concatenate([r, z, n, hn], axis=1)
    return out, hstate, saved


def gru_run_bwd(grad_out, grad_hn, hstate, saved, w_hh, seq_len=None, operand_round=None, dtype=F64):
    """BPTT of gru_run.  Returns dxproj [B,T,3H], dhproj [B,T,3H], dh0 [B,H] (dW_hh = sum_t dhproj_t^T hstate[:, t], db_hh = column sums)."""
    rnd = operand_round or _ident
    go, hs, sv, w = (np.asarray(a).astype(dtype) for a in (grad_out, hstate, saved, w_hh))
    b, t, h = go.shape
    w_op = rnd(w)
    dxproj = np.zeros((b, t, 3 * h), dtype=dtype)
    dhproj = np.zeros((b, t, 3 * h), dtype=dtype)
    carry = np.zeros((b, h), dtype=dtype) if grad_hn is None else np.asarray(grad_hn).reshape(b, h).astype(dtype)
    one = dtype(1)
    for s in range(t - 1, -1, -1):
        dstate = carry + (rnd(dhproj[:, s + 1]) @ w_op if s + 1 < t else 0)
        r, z, n, hn = (sv[:, s, g * h:(g + 1) * h] for g in range(4))
        hp = hs[:, s]
        dh = dstate + go[:, s]
        dn = dh * (one - z) * (one - n * n)
        dz = dh * (hp - n) * z * (one - z)
        dr = dn * hn * r * (one - r)
        act = _active(seq_len, s, b)[:, None]
        dxproj[:, s] = np.where(act, np.concatenate([dr, dz, dn], axis=1), 0)
        dhproj[:, s] = np.where(act, np.concatenate([dr, dz, dn * r], axis=1), 0)
        carry = np.where(act, dh * z, dstate)
    dh0 = carry + rnd(dhproj[:, 0]) @ w_op
    return dxproj, dhproj, dh0


def lstm_run(xproj, w_hh, b_hh, seq_len=None, h0=None, c0=None, operand_round=None, dtype=F64):
    """xproj [B,T,4H].  Returns out, hstate [B,T+1,H], cstate [B,T+1,H], saved [B,T,4H] = (i, f, g, o)."""
    rnd = operand_round or _ident
    x, w, bias = (np.asarray(a).astype(dtype) for a in (xproj, w_hh, b_hh))
    b, t, h4 = x.shape
    h = h4 // 4
    w_op = rnd(w)
    hstate = np.zeros((b, t + 1, h), dtype=dtype)
    cstate = np.zeros((b, t + 1, h), dtype=dtype)
    if h0 is not None:
        hstate[:, 0] = np.asarray(h0).reshape(b, h)
    if c0 is not None:
        cstate[:, 0] = np.asarray(c0).reshape(b, h)
    out = np.zeros((b, t, h), dtype=dtype)
    saved = np.zeros((b, t, 4 * h), dtype=dtype)
    for s in range(t):
        hp, cp = hstate[:, s], cstate[:, s]
        pre = x[:, s] + (rnd(hp) @ w_op.T + bias)
        i, f, o = _sig(pre[:, :h]), _sig(pre[:, h:2 * h]), _sig(pre[:, 3 * h:])
        g = np.tanh(pre[:, 2 * h:3 * h])
        cnew = f * cp + i * g
        hnew = o * np.tanh(cnew)
        act = _active(seq_len, s, b)[:, None]
        hstate[:, s + 1] = np.where(act, hnew, hp)
        cstate[:, s + 1] = np.where(act, cnew, cp)
        out[:, s] = np.where(act, hnew, 0)
        saved[:, s] = np.concatenate([i, f, g, o], axis=1)
    return out, hstate, cstate, saved


def lstm_run_bwd(grad_out, grad_hn, grad_cn, cstate, saved, w_hh, seq_len=None, operand_round=None, dtype=F64):
    """BPTT of lstm_run.  Returns dgates [B,T,4H], dh0, dc0 [B,H].  grad_out None = zero."""
    rnd = operand_round or _ident
    cs, sv, w = (np.asarray(a).astype(dtype) for a in (cstate, saved, w_hh))
    b, t, h = cs.shape[0], cs.shape[1] - 1, cs.shape[2]
    go = np.zeros((b, t, h), dtype=dtype) if grad_out is None else np.asarray(grad_out).astype(dtype)
    w_op = rnd(w)
    dgates = np.zeros((b, t, 4 * h), dtype=dtype)
    carry_h = np.zeros((b, h), dtype=dtype) if grad_hn is None else np.asarray(grad_hn).reshape(b, h).astype(dtype)
    carry_c = np.zeros((b, h), dtype=dtype) if grad_cn is None else np.asarray(grad_cn).reshape(b, h).astype(dtype)
    one = dtype(1)
    for s in range(t - 1, -1, -1):
        dh_state = carry_h + (rnd(dgates[:, s + 1]) @ w_op if s + 1 < t else 0)
        i, f, g, o = (sv[:, s, k * h:(k + 1) * h] for k in range(4))
        dh = dh_state + go[:, s]
        tc = np.tanh(cs[:, s + 1])
        dc = carry_c + dh * o * (one - tc * tc)
        act = _active(seq_len, s, b)[:, None]
        dg = np.concatenate([dc * g * i * (one - i), dc * cs[:, s] * f * (one - f), dc * i * (one - g * g), dh * tc * o * (one - o)], axis=1)
        dgates[:, s] = np.where(act, dg, 0)
        carry_h = np.where(act, 0, dh_state)
        carry_c = np.where(act, dc * f, carry_c)
    dh0 = carry_h + rnd(dgates[:, 0]) @ w_op
    return dgates, dh0, carry_c


# ------------------------------------------------------------------------------------------------------------ stacks, by composition
def gru_stack_run(xproj0, w_ih, w_hh, b_ih, b_hh, seq_len=None, h0s=None, operand_round=None, dtype=F64):
    """L stacked GRU layers: layer l >= 1 takes xproj = out_{l-1} W_ih[l]^T + b_ih[l].  Returns per-layer lists (out, hstate, saved)."""
    rnd = operand_round or _ident
    outs, hstates, saveds, xp = [], [], [], np.asarray(xproj0).astype(dtype)
    for l in range(len(w_hh)):
        if l > 0:
            xp = rnd(outs[-1]) @ rnd(np.asarray(w_ih[l]).astype(dtype)).T + np.asarray(b_ih[l]).astype(dtype)
        o, hs, sv = gru_run(xp, w_hh[l], b_hh[l], seq_len, None if h0s is None else h0s[l], operand_round, dtype)
        outs.append(o); hstates.append(hs); saveds.append(sv)
    return outs, hstates, saveds


def gru_stack_run_bwd(grad_out, grad_hn, hstates, saveds, w_ih, w_hh, seq_len=None, operand_round=None, dtype=F64):
    """BPTT of gru_stack_run, top layer first; dxin = dxproj W_ih is handed down.  Returns per-layer lists dxproj, dhproj, dh0."""
    rnd = operand_round or _ident
    n_layers = len(w_hh)
    dxp, dhp, dh0, go = [None] * n_layers, [None] * n_layers, [None] * n_layers, np.asarray(grad_out).astype(dtype)
    for l in range(n_layers - 1, -1, -1):
        dxp[l], dhp[l], dh0[l] = gru_run_bwd(go, None if grad_hn is None else grad_hn[l], hstates[l], saveds[l], w_hh[l], seq_len,
                                             operand_round, dtype)
        if l > 0:
            go = rnd(dxp[l]) @ rnd(np.asarray(w_ih[l]).astype(dtype))
    return dxp, dhp, dh0


def lstm_stack_run(xproj0, w_ih, w_hh, b_ih, b_hh, seq_len=None, h0s=None, c0s=None, operand_round=None, dtype=F64):
    """L stacked LSTM layers.  Returns per-layer lists (out, hstate, cstate, saved)."""
    rnd = operand_round or _ident
    res, xp = [], np.asarray(xproj0).astype(dtype)
    for l in range(len(w_hh)):
        if l > 0:
            xp = rnd(res[-1][0]) @ rnd(np.asarray(w_ih[l]).astype(dtype)).T + np.asarray(b_ih[l]).astype(dtype)
        res.append(lstm_run(xp, w_hh[l], b_hh[l], seq_len, None if h0s is None else h0s[l], None if c0s is None else c0s[l],
                            operand_round, dtype))
    return tuple(list(col) for col in zip(*res))


def lstm_stack_run_bwd(grad_out, grad_hn, grad_cn, cstates, saveds, w_ih, w_hh, seq_len=None, operand_round=None, dtype=F64):
    """BPTT of lstm_stack_run.  Returns per-layer lists dgates, dh0, dc0."""
    rnd = operand_round or _ident
    n_layers = len(w_hh)
    dg, dh0, dc0, go = [None] * n_layers, [None] * n_layers, [None] * n_layers, grad_out
    for l in range(n_layers - 1, -1, -1):
        dg[l], dh0[l], dc0[l] = lstm_run_bwd(go, None if grad_hn is None else grad_hn[l], None if grad_cn is None else grad_cn[l],
                                             cstates[l], saveds[l], w_hh[l], seq_len, operand_round, dtype)
        if l > 0:
            go = rnd(dg[l]) @ rnd(np.asarray(w_ih[l]).astype(dtype))
    return dg, dh0, dc0


# ------------------------------------------------------------------------------------------------------------ comparing
def ratio(got, want):
    """Worst |got - want.v| / want.e over the elements (0 where both the difference and the bound are 0); non-finite got -> inf."""
    got = np.asarray(got, dtype=F64)
    diff = np.abs(got - want.v)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(diff == 0, 0.0, diff / want.e)
    q = np.where(np.isfinite(got), q, np.inf)
    return float(q.max()) if q.size else 0.0


def rel_err(got, want):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


# ------------------------------------------------------------------------------------------------------------ step residuals
class Worst:
    """The largest observed / bound ratio of a run of step checks, and where it was seen (form, quantity, step, element)."""

    def __init__(self, form):
        self.form, self.ratio, self.where = form, 0.0, 'nothing compared'
        self.checks = 0

    def bounded(self, got, want, name, t, rows=None):
        got = np.asarray(got, dtype=F64)
        v, e = want.v, want.e
        if rows is not None:
            got, v, e = got[rows], v[rows], e[rows]
        if got.size == 0:
            return
        self.checks += 1
        diff = np.abs(got - v)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(diff == 0, 0.0, diff / e)
        q = np.where(np.isfinite(got), q, np.inf)
        k = int(np.argmax(q))
        if q.flat[k] > self.ratio:
            idx = np.unravel_index(k, q.shape)
            self.ratio = float(q.flat[k])
            self.where = '%s: %s at step %d, element %s: got %.9g want %.9g +- %.3g' % (self.form, name, t, tuple(int(i) for i in idx),
                                                                                          got.flat[k], v.flat[k], e.flat[k])

    def exact(self, got, want, name, t):
        got, want = np.asarray(got), np.asarray(want)
        if got.size == 0:
            return
        self.checks += 1
        bad = ~((got == want) & np.isfinite(got.astype(F64)))
        if bad.any():
            idx = np.unravel_index(int(np.argmax(bad)), bad.shape)
            self.ratio = float('inf')
            self.where = '%s: %s at step %d, element %s: got %r, must be exactly %r' % (self.form, name, t, tuple(int(i) for i in idx),
                                                                                       got[idx], want[idx])


def _t(a, t):
    return None if a is None else a[:, t]


def gru_forward_residual(form, xproj, w_op, b_hh, seq_len, hstate, h_operand, out, saved, fast=False, xproj_mag=None):
    """Every step of a GRU forward checked on its own from the stored inputs of that step.  h_operand [B,T+1,H]: what entered the
    product (hstate itself, or the bf16 shadow); w_op: the weight operand the kernel had.  Live steps: saved (r, z, n, hn) and
    hstate[:, t+1] within the bound, out[:, t] == hstate[:, t+1] exactly.  Padded steps: out == 0 and the state frozen, exactly; saved is
    not looked at (UNSPECIFIED by the header).  Returns a Worst."""
    worst = Worst(form)
    b, t_len, h = np.asarray(out).shape
    with np.errstate(all='ignore'):
        for t in range(t_len):
            act = _active(seq_len, t, b)
            st = gru_step(xproj[:, t], h_operand[:, t], hstate[:, t], w_op, b_hh, fast, _t(xproj_mag, t))
            for g, name in enumerate(('r', 'z', 'n', 'hn')):
                worst.bounded(saved[:, t, g * h:(g + 1) * h], st[name], 'saved.' + name, t, act)
            worst.bounded(hstate[:, t + 1], st['h_new'], 'hstate[t+1]', t, act)
            worst.exact(out[:, t][act], hstate[:, t + 1][act], 'out (live step) vs hstate[t+1]', t)
            worst.exact(out[:, t][~act], np.zeros_like(out[:, t][~act]), 'out (padded step)', t)
            worst.exact(hstate[:, t + 1][~act], hstate[:, t][~act], 'hstate[t+1] (padded step, frozen)', t)
    return worst


def gru_backward_residual(form, grad_out, grad_hn, hstate, saved, w_op, seq_len, dxproj, dhproj, dh_operand, dh0, grad_out_err=None):
    """Every step of a GRU BPTT checked from the kernel's own gate gradients of the step after it (dh_operand [B,T,3H]: dhproj, or its
    bf16 shadow) and the elementwise carry, which the kernels do not store: it is re-formed here in float64 from the quantities the
    previous step check has just verified (carry_t = dh_t z_t), its bound carried along.  The product is therefore one step deep; the
    carry's bound grows by one rounding per step and shrinks by z.  dxproj / dhproj may be None (forms that write shadows only)."""
    worst = Worst(form)
    b, t_len, h = np.asarray(grad_out).shape
    carry = Bounded(np.zeros((b, h)) if grad_hn is None else np.asarray(grad_hn, dtype=F64).reshape(b, h))
    with np.errstate(all='ignore'):
        for t in range(t_len - 1, -1, -1):
            act = _active(seq_len, t, b)
            dstate = state_grad(dh_operand[:, t + 1] if t + 1 < t_len else None, w_op, carry)
            go = Bounded(grad_out[:, t], 0.0 if grad_out_err is None else grad_out_err[:, t])
            g = gru_step_bwd(dstate, go, *(saved[:, t, k * h:(k + 1) * h] for k in range(4)), hstate[:, t], act)
            for k, (nx, nh) in enumerate((('dr', 'dr'), ('dz', 'dz'), ('dn', 'dnr'))):
                if dxproj is not None:
                    worst.bounded(dxproj[:, t, k * h:(k + 1) * h], g[nx], 'dxproj.' + nx, t)
                if dhproj is not None:
                    worst.bounded(dhproj[:, t, k * h:(k + 1) * h], g[nh], 'dhproj.' + nh, t)
            carry = g['carry']
        worst.bounded(dh0, state_grad(dh_operand[:, 0], w_op, carry), 'dh0', -1)
    return worst


def lstm_forward_residual(form, xproj, w_op, b_hh, seq_len, hstate, h_operand, cstate, out, saved, fast=False, xproj_mag=None,
                          hstate_rows_valid=True):
    """The LSTM twin of gru_forward_residual.  hstate_rows_valid=False: the form writes only slot T of hstate (the whole-stack launch);
    the per-step h is then checked through h_operand's next slot being the bf16 rounding of a value within the bound, and through out."""
    worst = Worst(form)
    b, t_len, h = np.asarray(cstate).shape[0], np.asarray(cstate).shape[1] - 1, np.asarray(cstate).shape[2]
    with np.errstate(all='ignore'):
        for t in range(t_len):
            act = _active(seq_len, t, b)
            st = lstm_step(xproj[:, t], h_operand[:, t], cstate[:, t], w_op, b_hh, fast, _t(xproj_mag, t))
            for g, name in enumerate(('i', 'f', 'g', 'o')):
                worst.bounded(saved[:, t, g * h:(g + 1) * h], st[name], 'saved.' + name, t, act)
            worst.bounded(cstate[:, t + 1], st['c_new'], 'cstate[t+1]', t, act)
            worst.exact(cstate[:, t + 1][~act], cstate[:, t][~act], 'cstate[t+1] (padded step, frozen)', t)
            if hstate_rows_valid:
                worst.bounded(hstate[:, t + 1], st['h_new'], 'hstate[t+1]', t, act)
                worst.exact(hstate[:, t + 1][~act], hstate[:, t][~act], 'hstate[t+1] (padded step, frozen)', t)
                if out is not None:
                    worst.exact(out[:, t][act], hstate[:, t + 1][act], 'out (live step) vs hstate[t+1]', t)
            else:
                # bf16 shadow of a value within the bound: widen by half a bf16 ulp of the value
                hb = Bounded(st['h_new'].v, st['h_new'].e + 2.0 ** -8 * np.abs(st['h_new'].v) + 2.0 ** -134)
                worst.bounded(np.asarray(h_operand[:, t + 1], dtype=F64), hb, 'hstate_bf[t+1]', t, act)
                worst.exact(np.asarray(h_operand[:, t + 1])[~act], np.asarray(h_operand[:, t])[~act], 'hstate_bf[t+1] (padded step, frozen)', t)
                if out is not None:
                    worst.bounded(out[:, t], st['h_new'], 'out', t, act)
            if out is not None:
                worst.exact(out[:, t][~act], np.zeros_like(out[:, t][~act]), 'out (padded step)', t)
    return worst


def lstm_backward_residual(form, grad_out, grad_hn, grad_cn, cstate, saved, w_op, seq_len, dgates, dg_operand, dh0, dc0, grad_out_err=None,
                           fast=False):
    """The LSTM twin of gru_backward_residual: the elementwise carry is d loss / d c (carry_c = dc_t f_t); all of d loss / d h_{t-1} of
    a live step is the product dg_operand[:, t] @ w_op.  grad_out None = zero; dgates None = the form writes the bf16 shadow only."""
    worst = Worst(form)
    b, t_len, h = np.asarray(cstate).shape[0], np.asarray(cstate).shape[1] - 1, np.asarray(cstate).shape[2]
    carry_h = Bounded(np.zeros((b, h)) if grad_hn is None else np.asarray(grad_hn, dtype=F64).reshape(b, h))
    carry_c = Bounded(np.zeros((b, h)) if grad_cn is None else np.asarray(grad_cn, dtype=F64).reshape(b, h))
    with np.errstate(all='ignore'):
        for t in range(t_len - 1, -1, -1):
            act = _active(seq_len, t, b)
            dh_state = state_grad(dg_operand[:, t + 1] if t + 1 < t_len else None, w_op, carry_h)
            go = Bounded(np.zeros((b, h)) if grad_out is None else grad_out[:, t], 0.0 if grad_out_err is None else grad_out_err[:, t])
            g = lstm_step_bwd(dh_state, carry_c, go, *(saved[:, t, k * h:(k + 1) * h] for k in range(4)), cstate[:, t], cstate[:, t + 1], act, fast)
            if dgates is not None:
                for k, name in enumerate(('di', 'df', 'dg', 'do')):
                    worst.bounded(dgates[:, t, k * h:(k + 1) * h], g[name], 'dgates.' + name, t)
            carry_h, carry_c = g['carry_h'], g['carry_c']
        worst.bounded(dh0, state_grad(dg_operand[:, 0], w_op, carry_h), 'dh0', -1)
        worst.bounded(dc0, carry_c, 'dc0', -1)
    return worst
