"""torch-facing wrappers of the two custom HIP policy ops (include/ic3_rollout.h).  No CPU fallback."""
import ctypes as C
from functools import partial

import torch

from . import _lib
from ._lib import check, int32_array, ptr, stream


def _need_cuda(t, name):
    if not t.is_cuda:
        raise _lib.IC3Error("%s: expected a CUDA (ROCm) tensor — the HIP op has no CPU fallback" % name)


def _dense(t, shape=None, dtype=None, none_ok=False):
    """What the wrappers assert of a buffer: a contiguous tensor, of `dtype` when given, of `shape` when given (a tuple: the
    shape itself; an int: that many elements).  None passes only where the argument is optional (`none_ok`)."""
    if t is None:
        return none_ok
    if not t.is_contiguous() or (dtype is not None and t.dtype != dtype):
        return False
    if shape is None:
        return True
    return t.numel() == shape if isinstance(shape, int) else t.shape == shape


_f32 = partial(_dense, dtype=torch.float32)
_i32 = partial(_dense, dtype=torch.int32)


def _mask(m, R, none_ok=True):
    """An int32 row mask (alive / gate) of R rows, or None: nobody masked."""
    return _i32(m, R, none_ok=none_ok)


def _set_ptrs(struct, tensors=(), **optional):
    """struct.<field> = the tensor's device pointer for every field named: `tensors`, a dict, holds the arguments that must be
    tensors; the keyword ones may be None (-> NULL)."""
    for name in tensors:
        setattr(struct, name, tensors[name].data_ptr())
    for name, t in optional.items():
        setattr(struct, name, None if t is None else t.data_ptr())


class _CommMaskedMean(torch.autograd.Function):
    """comm.py:181-205 in closed form.  The map h -> out is linear with a symmetric (N x N) mixing matrix
    M[j,i] = m_j m_i s (i != j), so the backward pass is the same kernel applied to grad_out."""

    @staticmethod
    def forward(ctx, h, alive, comm_action, mode_avg, mask_self):
        ctx.alive, ctx.comm_action, ctx.mode_avg, ctx.mask_self = alive, comm_action, mode_avg, mask_self
        return comm_masked_mean_raw(h, alive, comm_action, mode_avg, mask_self)

    @staticmethod
    def backward(ctx, g):
        return comm_masked_mean_raw(g.contiguous(), ctx.alive, ctx.comm_action, ctx.mode_avg, ctx.mask_self), None, None, None, None


class _EnvEncode(torch.autograd.Function):
    """encoder(obs(env state)) with a backward: forward = the sparse gather ic3_env_encode, backward = the
    position-sum scatter ic3_env_encode_backward on a snapshot of the integer state (no dense obs is kept)."""

    @staticmethod
    def forward(ctx, weight, bias, env, weight_t, loc_table):
        out = env.encode(weight_t, bias.detach(), loc_table=loc_table)
        ctx.env = env
        ctx.snap = env.snapshot()
        ctx.need_bias = bias.requires_grad
        return out

    @staticmethod
    def backward(ctx, g):
        dwt, dbias = ctx.env.encode_backward(g.contiguous(), ctx.snap, want_bias=ctx.need_bias)
        return dwt.t().contiguous(), dbias, None, None, None      # contiguous: grads may be all-reduced (sharding.py)


def env_encode(env, weight, bias, weight_t=None, loc_table=None):
    """nn.Linear(obs_dim, H)(env's current observation) -> (E, N, H), differentiable w.r.t. weight (H, obs_dim) and
    bias; weight_t = weight.t().contiguous() if the caller caches it."""
    if weight_t is None:
        weight_t = weight.detach().t().contiguous()
    return _EnvEncode.apply(weight, bias, env, weight_t, loc_table)


def _rows(t, H):
    """(tensor usable by the kernels, row stride in floats) for a (..., H) fp32 tensor whose rows are unit-stride
    and evenly spaced (e.g. a column slice of a wider row-major buffer); anything else is made contiguous."""
    if t.dtype != torch.float32:
        t = t.float()
    flat = t.reshape(-1, H) if t.is_contiguous() else t
    if flat.dim() == 2 and flat.stride(1) == 1 and flat.stride(0) >= H:
        return flat, flat.stride(0)
    if t.dim() == 3 and t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1) and t.stride(1) >= H:
        return t, t.stride(1)
    t = t.contiguous()
    return t, H


def comm_masked_mean_raw(h, alive, comm_action, mode_avg, mask_self, out=None, addend=None, row_scale=None):
    """The kernel launch without autograd: h (E,N,H) rows may be a strided column slice; `out` (E,N,H) contiguous.
    `addend` (E*N,H) / (E,N,H) rows (a strided column slice is fine): out = addend + comm(h) (ic3_comm_masked_mean_add);
    `row_scale` (E*N,) float32 with it: every output row times its factor."""
    _need_cuda(h, "comm_masked_mean")
    E, N, H = h.shape
    hk, ldh = _rows(h, H)
    if out is None:
        out = torch.empty((E, N, H), dtype=torch.float32, device=h.device)
    if addend is not None:
        ak, lda = _rows(addend, H)
        assert _f32(row_scale, E * N, none_ok=True)
        check(_lib.lib().ic3_comm_masked_mean_add(ptr(hk), ldh, ptr(alive), ptr(comm_action), ptr(ak), lda, ptr(row_scale), ptr(out),
                                                  E, N, H, int(mode_avg), int(mask_self), stream()))
        return out
    assert row_scale is None, "row_scale comes with an addend"
    check(_lib.lib().ic3_comm_masked_mean(ptr(hk), ldh, ptr(alive), ptr(comm_action), ptr(out), E, N, H,
                                          int(mode_avg), int(mask_self), stream()))
    return out


def lstm_cell_(gates, c, h_out):
    """In-place LSTM pointwise step: gates (R,4H) contiguous, c (R,H) contiguous (updated), h_out (R,H) rows
    with unit column stride (may be a column slice of a wider buffer)."""
    _need_cuda(gates, "lstm_cell")
    R, H = c.shape
    assert _dense(gates) and _dense(c) and h_out.stride(1) == 1
    check(_lib.lib().ic3_lstm_cell(ptr(gates), ptr(c), ptr(h_out), h_out.stride(0), R, H, stream()))
    return h_out, c


LSTM_BWD_MAX_PARTIALS = 2048


def lstm_cell_backward(gates, c_prev, dh, dc, dgates, dc_prev, dbias_partials=None):
    """Backward of lstm_cell_ from the re-computed gate pre-activations (ic3_lstm_cell_backward): gates (R,4H), c_prev,
    dh, dc (or None) (R,H) -> dgates (R,4H), dc_prev (R,H; may alias dc).  dbias_partials: (LSTM_BWD_MAX_PARTIALS, 4H)
    scratch — returns the view of the rows the call wrote (their sum over dim 0 = column sums of dgates), else None.
    All contiguous float32."""
    _need_cuda(gates, "lstm_cell_backward")
    R, H = c_prev.shape
    for t in (gates, c_prev, dh, dgates, dc_prev):
        assert _f32(t)
    assert _dense(dbias_partials, (LSTM_BWD_MAX_PARTIALS, 4 * H), none_ok=True)
    n = check(_lib.lib().ic3_lstm_cell_backward(ptr(gates), ptr(c_prev), ptr(dh), ptr(dc), ptr(dgates), ptr(dc_prev),
                                                ptr(dbias_partials), R, H, stream()))
    return dbias_partials[:n] if dbias_partials is not None else None


def commnet_forward_supported(H, N):
    return bool(_lib.lib().ic3_commnet_forward_supported(int(H), int(N)))


def _commnet_pack_passes(entry, c_weights, f_weights, out):
    """out[i] <- entry([C_i | F_i]) for every communication pass i."""
    H = c_weights[0].shape[0]
    for i in range(len(c_weights)):
        check(entry(ptr(c_weights[i].detach().contiguous().float()), ptr(f_weights[i].detach().contiguous().float()), ptr(out[i]), H,
                    stream()))
    return out


def commnet_pack(c_weights, f_weights, c_biases, f_biases):
    """Per-pass [C_i | F_i] in the layout ic3_commnet_forward streams + the summed biases: lists of (H,H) / (H,) tensors."""
    _need_cuda(c_weights[0], "commnet_pack")
    H, P, dev = c_weights[0].shape[0], len(c_weights), c_weights[0].device
    wp = _commnet_pack_passes(_lib.lib().ic3_commnet_pack, c_weights, f_weights,
                              torch.empty((P, 2 * H * H), dtype=torch.float32, device=dev))
    bias = torch.stack([(c_biases[i] + f_biases[i]).detach().float() for i in range(P)]).contiguous()
    return wp, bias


def commnet_pack_split(c_weights, f_weights):
    """Per-pass [C_i | F_i] as three exact bf16 planes in MFMA fragment order (ic3_commnet_pack_split): (P, 3 * H * H) float32
    words, or None when hid_size is not a multiple of 32."""
    H, P, dev = c_weights[0].shape[0], len(c_weights), c_weights[0].device
    if H % 32:
        return None
    return _commnet_pack_passes(_lib.lib().ic3_commnet_pack_split, c_weights, f_weights,
                                torch.empty((P, 3 * H * H), dtype=torch.float32, device=dev))


def commnet_forward(enc, E, N, wp, bias, head_w, head_b, head_sizes, mode_avg, comm_zero, alive_in, comm_in, out=None,
                    h_out=None, wp3=None):
    """The non-recurrent CommNet module after the encoder, every communication pass in one launch (ic3_commnet_forward):
    enc (E*N, H) = encoder(obs) incl. bias -> out (E*N, OT) = [log-probs of every head | value]."""
    _need_cuda(enc, "commnet_forward")
    R, H = enc.shape
    assert R == E * N and _f32(enc)
    assert _mask(alive_in, R) and _mask(comm_in, R)
    OT = sum(int(a) for a in head_sizes) + 1
    if out is None:
        out = torch.empty((R, OT), dtype=torch.float32, device=enc.device)
    sizes = int32_array(head_sizes)
    assert _dense(wp3, (wp.shape[0], 3 * H * H), none_ok=True)
    check(_lib.lib().ic3_commnet_forward(ptr(enc), E, N, H, wp.shape[0], ptr(wp), ptr(wp3), ptr(bias), ptr(head_w), ptr(head_b), sizes,
                                         len(head_sizes), int(bool(mode_avg)), int(bool(comm_zero)), ptr(alive_in),
                                         ptr(comm_in), ptr(out), ptr(h_out), stream()))
    return out


def commnet_step_supported(env, H):
    return _lib.lib().ic3_commnet_step_supported(env._h, int(H)) > 0


def commnet_step(env, cn, H, head_sizes, mode_avg, comm_zero, alive_in, comm_in, out, action, reward, done, alive=None,
                 is_completed=None, obs=None, h_in=None, h_out=None):
    """One whole rollout iteration of the NON-recurrent module (sparse encoder -> communication passes -> heads -> draws ->
    env.step, + the dense obs rows of the state acted on) in one launch — ic3_commnet_step.  `cn`: the module's derived
    weights (wt, enc_bias, loc_table, wp, bias, w_heads, b_heads; wp3 = the split planes or None: the fp32 instruction)."""
    _need_cuda(out, "commnet_step")
    R = out.shape[0]
    assert _dense(out) and _i32(action, len(head_sizes) * R) and out.shape[1] == sum(int(a) for a in head_sizes) + 1
    assert _mask(alive_in, R) and _mask(comm_in, R)
    assert _f32(h_in, R * int(H), none_ok=True) and _f32(h_out, R * int(H), none_ok=True)
    sizes = int32_array(head_sizes)
    check(_lib.lib().ic3_commnet_step(env._h, ptr(cn['wt']), ptr(cn['enc_bias']), ptr(cn['loc_table']), int(H),
                                      cn['wp'].shape[0], ptr(cn['wp']), ptr(cn.get('wp3')), ptr(cn['bias']), ptr(cn['w_heads']),
                                      ptr(cn['b_heads']),
                                      sizes, len(head_sizes), int(bool(mode_avg)), int(bool(comm_zero)), ptr(alive_in),
                                      ptr(comm_in), ptr(h_in), ptr(h_out), ptr(out), ptr(action), ptr(obs), ptr(reward), ptr(done),
                                      ptr(alive), ptr(is_completed), stream()))
    return out


def lstm_gates_backward_supported(H):
    return bool(_lib.lib().ic3_lstm_gates_backward_supported(int(H)))


def lstm_gates_backward(xh, lstm_wp, bias, c_prev, dh, dc, dgates, dc_prev, dbias_partials=None, accumulate=False,
                        h_prev=None, lstm_wp3=None, lstm_wp3_bwd=None, dxh=None):
    """Gate recompute + LSTM cell backward in one launch (ic3_lstm_gates_backward): xh (R,2H) = [inp | h_prev] rows (unit
    column stride; with h_prev (R,H) given the launch fills the h half of xh from it), lstm_wp = policy_step_pack's 'ps_l_wp', bias (4H,) = b_ih + b_hh; c_prev, dh, dc (or None) (R,H) ->
    dgates (R,4H), dc_prev (R,H; may alias dc).  dbias_partials: (ceil(R/64), 4H), written (or added to: `accumulate`).
    lstm_wp3: the split gate product.  dxh (R,2H) with lstm_wp3 and lstm_wp3_bwd: + the input gradient [d inp | d h_prev] =
    dgates . [W_ih | W_hh] in the same launch (ic3_lstm_gates_backward_dx)."""
    _need_cuda(xh, "lstm_gates_backward")
    R, H = c_prev.shape
    assert xh.dtype == torch.float32 and xh.stride(1) == 1 and xh.shape == (R, 2 * H)
    for t in (c_prev, dh, dgates, dc_prev, bias, lstm_wp):
        assert _f32(t)
    assert _dense(dbias_partials, ((R + 63) // 64, 4 * H), none_ok=True)
    assert _f32(h_prev, (R, H), none_ok=True)
    entry, bwd_planes, dx = _lib.lib().ic3_lstm_gates_backward, (), ()
    if dxh is not None:
        assert lstm_wp3 is not None and lstm_wp3_bwd is not None and _dense(dxh, (R, 2 * H))
        entry, bwd_planes, dx = _lib.lib().ic3_lstm_gates_backward_dx, (ptr(lstm_wp3_bwd),), (ptr(dxh),)
    return check(entry(ptr(xh), xh.stride(0), ptr(h_prev), ptr(lstm_wp), ptr(lstm_wp3), *bwd_planes, ptr(bias), ptr(c_prev), ptr(dh),
                       ptr(dc), ptr(dgates), ptr(dc_prev), ptr(dbias_partials), int(bool(accumulate)), *dx, R, H, stream()))


def _rowvec(v, R):
    assert _f32(v, R, none_ok=True)
    return ptr(v)


def lstm_gates_backward_given(gates, c_prev, dh, dc, dgates, dc_prev, dbias_partials=None, accumulate=False, xh=None,
                              h_prev=None, lstm_wp3_bwd=None, dxh=None, row_live=None, row_keep=None, dhead=None, w_heads=None):
    """The cell's derivative from the RECORDED activated gates (R, 4H) of the step (ic3_lstm_gates_backward_given; the
    rollout's launch stored them: envs.set_record_out) — no gate product.  xh + h_prev: h_prev is copied into the h half of xh;
    lstm_wp3_bwd + dxh: [d inp | d h_prev] in the same launch.  row_live / row_keep (R,) float32 (collection mode): c_prev and
    the copied h_prev times row_live, dc times row_keep, per row.  dgates may be `gates` itself (in place).  dhead (R, OT) +
    w_heads (OT, H): dh + dhead @ w_heads is what the cell sees (the heads' share of dL/dh_t, folded in).  dh and / or dc None:
    zeros (a detach point of the recurrence; no buffer is read) — dh None needs dhead, row_keep needs dc."""
    _need_cuda(gates, "lstm_gates_backward_given")
    R, H = c_prev.shape
    for t in (gates, c_prev, dgates, dc_prev):
        assert _f32(t)
    assert _f32(dh, none_ok=True) and _f32(dc, none_ok=True)
    assert dh is not None or dhead is not None      # (dh None = zeros: a detach point, the heads' share alone reaches the cell)
    assert tuple(gates.shape) == (R, 4 * H) and tuple(dgates.shape) == (R, 4 * H)
    assert _dense(dbias_partials, ((R + 63) // 64, 4 * H), none_ok=True)
    ldxh = 0
    if xh is not None:
        assert h_prev is not None and xh.dtype == torch.float32 and xh.stride(1) == 1 and xh.shape == (R, 2 * H)
        assert _dense(h_prev, (R, H))
        ldxh = xh.stride(0)
    if dxh is not None:
        assert lstm_wp3_bwd is not None and _dense(dxh, (R, 2 * H))
    OT = 0
    if dhead is not None:
        OT = dhead.shape[1]
        assert w_heads is not None and _f32(dhead) and dhead.shape[0] == R
        assert _f32(w_heads, (OT, H))
    # three arguments count only beside another one: without it the library is handed NULL whatever the caller passed
    h_prev = h_prev if xh is not None else None                    # (copied into xh)
    lstm_wp3_bwd = lstm_wp3_bwd if dxh is not None else None       # (the product that fills dxh)
    w_heads = w_heads if dhead is not None else None               # (dhead's weights)
    return check(_lib.lib().ic3_lstm_gates_backward_given(ptr(gates), ptr(xh), ldxh, ptr(h_prev), ptr(lstm_wp3_bwd), ptr(c_prev), ptr(dh),
                                                          ptr(dc), ptr(dgates), ptr(dc_prev), ptr(dbias_partials),
                                                          int(bool(accumulate)), ptr(dxh), _rowvec(row_live, R), _rowvec(row_keep, R),
                                                          ptr(dhead), ptr(w_heads), OT, R, H, stream()))


def comm_backward_partials(E, N):
    return int(_lib.lib().ic3_comm_backward_partials(int(E), int(N)))


def comm_backward(dxh, h_prev, alive, gate, c_weight, dh_out, dcw_partials, E, N, mode_avg=True, comm_zero=False,
                  out_scale=None, accumulate=True):
    """ic3_comm_backward: dh_out (R, H) = (dxh[:, H:] + mix(dxh[:, :H]) @ c_weight) * out_scale and dcw_partials (P, H, H)
    (+)= per-workgroup partial sums of mix(d inp)^T @ h_prev — the communication block's and C's share of one recorded step's
    backward in one launch.  comm_zero: dh_out = dxh[:, H:] * out_scale."""
    _need_cuda(dxh, "comm_backward")
    R, H2 = dxh.shape
    H = H2 // 2
    assert R == E * N and _f32(dxh) and _dense(dh_out, (R, H))
    if not comm_zero:
        assert _dense(h_prev, (R, H)) and _dense(c_weight, (H, H))
        assert _dense(dcw_partials, (comm_backward_partials(E, N), H, H))
        assert _mask(alive, R) and _mask(gate, R)
    return check(_lib.lib().ic3_comm_backward(ptr(dxh), 2 * H, ptr(h_prev), ptr(alive), ptr(gate), ptr(c_weight), _rowvec(out_scale, R),
                                              ptr(dh_out), ptr(dcw_partials), int(bool(accumulate)), E, N, H, int(bool(mode_avg)),
                                              int(bool(comm_zero)), stream()))


def _scratch(work, key, n, device):
    """A float32 scratch tensor of at least n elements on `device`, kept in the caller's dict `work` under (key, device) and grown
    when a call needs more (work None: a fresh one)."""
    work = work if work is not None else dict()
    key = (key, str(device))
    if key not in work or work[key].numel() < n:
        work[key] = torch.empty((n,), dtype=torch.float32, device=device)
    return work[key]


def lstm_weight_grad(inp, h_prev, dgates, dW, row_live=None, accumulate=True, work=None, split=True):
    """ic3_lstm_weight_grad_wide: dW (2H, 4H) (+)= [inp | h_prev]^T @ dgates over all Q rows of a window of recorded steps in one
    launch.  inp (Q, >= H) rows with unit column stride (the first H floats count: the record's [inp | h] rows), h_prev (Q, H),
    dgates (Q, 4H) contiguous; leading dims may be (T, R).  split (default): exact bf16 split products on the bf16 matrix cores
    (the rollout's gate_split arithmetic); False: the fp32 matrix instruction."""
    _need_cuda(dgates, "lstm_weight_grad")
    H = h_prev.shape[-1]
    Q = dgates.numel() // (4 * H)
    inp2 = inp.reshape(Q, inp.shape[-1])
    assert inp2.stride(1) == 1 and inp2.shape[1] >= H and inp2.dtype == torch.float32
    assert _dense(h_prev, Q * H) and _f32(dgates)
    assert _dense(dW, (2 * H, 4 * H))
    assert _f32(row_live, Q, none_ok=True)
    n = int(_lib.lib().ic3_lstm_weight_grad_wide_scratch_floats(Q, H, inp2.stride(0)))
    if n == 0:
        raise NotImplementedError("lstm_weight_grad: hid_size 64 / 128 / 256")
    check(_lib.lib().ic3_lstm_weight_grad_wide(ptr(inp2), inp2.stride(0), ptr(h_prev), ptr(dgates), ptr(row_live), Q, H, ptr(dW),
                                               int(bool(accumulate)), int(bool(split)), ptr(_scratch(work, 'wgrad', n, dgates.device)),
                                               stream()))


def first_chain_envs(E, N):
    """ic3_bptt_first_chain_envs: with ic3_bptt.two_chains, envs [0, E1) run on the caller's stream and [E1, E) on a second one."""
    return int(_lib.lib().ic3_bptt_first_chain_envs(int(E), int(N)))


def bptt_dcw_partials(E, N, two_chains):
    """Slots of ic3_bptt.dcw_partials."""
    E1 = first_chain_envs(E, N) if two_chains else E
    return comm_backward_partials(E1, N) + (comm_backward_partials(E - E1, N) if E1 < E else 0)


def bptt_backward_supported(env, H):
    return bool(_lib.lib().ic3_bptt_backward_supported(env._h, int(H)))


def bptt_passes_backward_supported(env, H, passes):
    """bptt_passes_backward can run: what ic3_bptt_backward needs, the encoder backward's window form, at least two passes."""
    return passes >= 2 and bptt_backward_supported(env, H) and env.encode_window_work(H) is not None


def bptt_passes_backward(env, T, E, N, H, gates, hs, cs, dhead, snaps, alive, gate, lstm_wp3_bwd, w_heads, c_weights, dh, dc, dxh,
                         dbias_partials, dcw_partials, mode_avg=True, comm_zero=False, detach_gap=0, t_first=0, enc_first=True,
                         row_keep=None, keep_before=None):
    """ic3_bptt_backward on an ic3_bptt_passes descriptor: the backward through T recorded steps of a comm_passes = P > 1 policy (a window, or a chunk of whole
    steps of one starting at its step t_first) as one host call.  Per pass i, lists of P tensors: gates[i] (T, R, 4H) — the record
    ops.policy_forward_record left, dgates on return —, hs[i] / cs[i] (T, R, H) the state entering the pass, dxh[i] (T, R, 2H) the
    ring of input gradients (written), dbias_partials[i] (ceil(R / 64), 4H) and dcw_partials[i] (comm_backward_partials(E, N), H, H)
    added to, c_weights[i] (H, H) (dcw_partials / c_weights: None with comm_zero).  alive / gate: lists of T (E, N) int32 tensors or
    None entries, or None.  The encoder's window stage runs behind the loop (finish: env.encode_backward_window_finish).
    Collection mode: row_keep (T, R) = keep of the call's slots, keep_before (R,) = keep of the slot in front of the call's first one
    (None at a window's first slot); hs[0] / cs[0] are then the caller's copies with the starting envs' rows zeroed."""
    _need_cuda(dh, "bptt_passes_backward")
    assert _f32(row_keep, T * E * N, none_ok=True) and _f32(keep_before, E * N, none_ok=True)
    R = E * N
    P = len(gates)
    assert P >= 2 and len(hs) == len(cs) == len(dxh) == len(dbias_partials) == P
    OT = _window_inputs(dhead, snaps, T, R)
    assert _f32(dh, (R, H)) and _f32(dc, (R, H))
    for i in range(P):
        assert _f32(gates[i], T * R * 4 * H) and _f32(hs[i], T * R * H) and _f32(cs[i], T * R * H)
        assert _f32(dxh[i], (T, R, 2 * H)) and _f32(dbias_partials[i], ((R + 63) // 64, 4 * H))
    if not comm_zero:
        assert len(c_weights) == len(dcw_partials) == P
        assert all(_f32(c_weights[i], (H, H)) and _f32(dcw_partials[i], (comm_backward_partials(E, N), H, H)) for i in range(P))

    def ptrs(ms, n, masks=False):
        if ms is None or (masks and all(m is None for m in ms)):
            return None
        assert len(ms) >= n and (not masks or all(_mask(m, R) for m in ms[:n]))
        return (C.c_void_p * n)(*[None if m is None else m.data_ptr() for m in ms[:n]])
    arrays = dict(gates=ptrs(gates, P), hs=ptrs(hs, P), cs=ptrs(cs, P), dxh=ptrs(dxh, P), dbias_partials=ptrs(dbias_partials, P),
                  c_weight=None if comm_zero else ptrs(c_weights, P), dcw_partials=None if comm_zero else ptrs(dcw_partials, P),
                  alive=ptrs(alive, T, True), gate=ptrs(gate, T, True))          # (alive until the call has returned)
    b = _lib.BpttPasses(T, E, N, H, OT, P, int(bool(mode_avg)), int(bool(comm_zero)), int(detach_gap), int(bool(enc_first)), int(t_first))
    for name, arr in arrays.items():
        setattr(b, name, C.cast(arr, C.POINTER(C.c_void_p)) if arr is not None else None)
    _set_ptrs(b, dict(dhead=dhead, snaps=snaps, lstm_wp3_bwd=lstm_wp3_bwd, w_heads=w_heads, dh=dh, dc=dc),
              row_keep=row_keep, keep_before=keep_before)
    b.snap_words = snaps.stride(0)
    b.dxh_step = dxh[0].stride(0)
    assert all(d.stride(0) == b.dxh_step for d in dxh)
    b.enc_work = _enc_work(env, H, True)
    check(_lib.lib().ic3_bptt_backward(env._h, C.byref(b), stream()))      # (its magic says which descriptor this is)


def record_xh_width(H):
    """Row width of the inp record ic3_env_set_record_out writes: 2H ([inp | h] rows, the h half left to the backward) at hid
    64 / 128, H (inp rows alone) at hid 256."""
    return H if H == 256 else 2 * H


# ---- what the four window backwards (ic3_bptt_backward, ic3_rnn_backward_wide, ic3_mlp_backward_wide, ic3_commnet_backward) share
def _window_inputs(dhead, snaps, T, R):
    """The checks of dhead (T, R, OT) and of the state snapshots snaps (>= T, words); returns OT."""
    OT = dhead.shape[-1]
    assert _f32(dhead, T * R * OT)
    assert _i32(snaps) and snaps.shape[0] >= T
    return OT


def _enc_work(env, H, window):
    """Device pointer of the encoder backward's partial sums: the window form's, or the per-step form's."""
    return (env.encode_window_work(H) if window else env._encb_work(H)).data_ptr()


def _a2_grad_fill(b, a2_grad, work, Q, H, device):
    """affine2's weight gradient over a window's Q rows (ic3_rnn_bptt / ic3_mlp_bptt: a2_grad + wgrad_scratch).  Returns the
    scratch tensor: the caller holds it until the call has returned."""
    if a2_grad is None:
        return None
    assert _f32(a2_grad, (H, H))
    scratch = _scratch(work, 'rnn_wgrad', int(_lib.lib().ic3_rnn_weight_grad_wide_scratch_floats(Q, H)), device)
    _set_ptrs(b, dict(a2_grad=a2_grad, wgrad_scratch=scratch))
    return scratch


def bptt_backward(env, T, E, N, H, gates, hs, cs, dhead, snaps, alive, gate, lstm_wp3_bwd, w_heads, c_weight, dh, dc, dxh,
                  dbias_partials, dcw_partials, mode_avg=True, comm_zero=False, detach_gap=0, row_live=None, row_keep=None,
                  enc_first=True, gate_events=None, two_chains=False, walk=False, max_workgroups=0):
    """ic3_bptt_backward: the backward through a window of T recorded steps as one host call (gate launch in place on the
    record, communication backward, encoder backward stage 1 — three launches per step).  alive / gate: lists of T tensors
    (E, N) int32 or None entries, or None.  gate_events: a list that receives (start, stop, t) DispatchEvent triples stamped
    around every step's gate launch (measurement: bench.py --mode train).
    walk: a comm_zero window with the ring, its T steps in ONE launch (an ic3_bptt_walk descriptor: every 64-row tile walked last
    step to first by one workgroup, dL/dh on chip) — the same dgates, d inp columns of the ring, dh, dc and bias partials bit for
    bit; the d h_prev columns of the ring are not written.  max_workgroups > 0 caps that launch's grid (0: the library's plan)."""
    if walk:
        if not comm_zero:
            raise ValueError("bptt_backward: walk=True needs comm_zero=True (a communicating policy's rows depend on each other)")
        if dxh.dim() != 3:
            raise ValueError("bptt_backward: walk=True needs the ring of per-step input gradients, dxh (T, R, 2H)")
        if gate_events is not None:
            raise ValueError("bptt_backward: walk=True is one launch: there are no per-step gate events")
    _need_cuda(gates, "bptt_backward")
    R = E * N
    assert _f32(gates, T * R * 4 * H)
    assert _dense(hs) and _dense(cs) and hs.shape[0] >= T and tuple(hs.shape[1:]) == (R, H) == tuple(cs.shape[1:])
    OT = _window_inputs(dhead, snaps, T, R)
    assert _f32(dh, (R, H)) and _f32(dc, (R, H))
    assert _dense(dxh) and tuple(dxh.shape) in ((R, 2 * H), (T, R, 2 * H))      # one buffer, or a ring of T (dxh_step)
    assert _dense(dbias_partials, ((R + 63) // 64, 4 * H))
    ring = dxh.dim() == 3
    two_chains = bool(two_chains) and ring and first_chain_envs(E, N) < E
    if not comm_zero:
        assert _dense(dcw_partials, (bptt_dcw_partials(E, N, two_chains), H, H))
        assert _dense(c_weight, (H, H))
    assert _f32(row_live, (T, R), none_ok=True) and _f32(row_keep, (T, R), none_ok=True)
    if walk:      # (no masks, no C, one stream: the fields a comm_zero window uses)
        b = _lib.BpttWalk(T, E, N, H, OT, int(detach_gap), int(bool(enc_first)), int(max_workgroups))
        _set_ptrs(b, dict(gates=gates, hs=hs, cs=cs, dhead=dhead, snaps=snaps, lstm_wp3_bwd=lstm_wp3_bwd, w_heads=w_heads, dh=dh, dc=dc,
                          dxh=dxh, dbias_partials=dbias_partials),
                  row_live=row_live, row_keep=row_keep)
        b.snap_words = snaps.stride(0)
        b.dxh_step = dxh.stride(0)
        b.enc_work = _enc_work(env, H, True)
        check(_lib.lib().ic3_bptt_backward(env._h, C.byref(b), stream()))      # (its magic says which descriptor this is)
        return

    def ptrs(ms):
        if ms is None or all(m is None for m in ms):
            return None
        assert len(ms) >= T
        assert all(_mask(m, R) for m in ms[:T])
        return (C.c_void_p * T)(*[None if m is None else m.data_ptr() for m in ms[:T]])
    pa, pg = ptrs(alive), ptrs(gate)                # (alive until the call has returned)
    b = _lib.Bptt(T, E, N, H, OT, int(bool(mode_avg)), int(bool(comm_zero)), int(detach_gap), int(bool(enc_first)))
    _set_ptrs(b, dict(gates=gates, hs=hs, cs=cs, dhead=dhead, snaps=snaps, lstm_wp3_bwd=lstm_wp3_bwd, w_heads=w_heads, dh=dh, dc=dc,
                      dxh=dxh, dbias_partials=dbias_partials),
              row_live=row_live, row_keep=row_keep, c_weight=c_weight, dcw_partials=dcw_partials)
    b.snap_words = snaps.stride(0)
    b.alive = C.cast(pa, C.POINTER(C.c_void_p)) if pa is not None else None
    b.gate = C.cast(pg, C.POINTER(C.c_void_p)) if pg is not None else None
    b.two_chains = int(two_chains)
    if ring:                               # a ring of per-step input gradients: the encoder's first stage once, over the window
        b.dxh_step = dxh.stride(0)
    b.enc_work = _enc_work(env, H, ring)
    evs = None
    if gate_events is not None:
        from .envs import DispatchEvent
        evs = [DispatchEvent() for _ in range(2 * T)]
        arr = (C.c_void_p * (2 * T))(*[e.handle.value for e in evs])
        b.gate_events = C.cast(arr, C.POINTER(C.c_void_p))
    check(_lib.lib().ic3_bptt_backward(env._h, C.byref(b), stream()))
    if evs is not None:
        gate_events.extend((evs[2 * t], evs[2 * t + 1], t) for t in range(T))


def rnn_backward_supported(env, H):
    """ic3_rnn_backward_wide_supported: the tanh-recurrence baseline's window backward runs for this env handle at hid_size H."""
    return bool(_lib.lib().ic3_rnn_backward_wide_supported(env._h, int(H)))


def rnn_backward_partials(R, H):
    """Rows of ic3_rnn_bptt.dbias_partials (ic3_rnn_backward_wide_partials)."""
    return int(_lib.lib().ic3_rnn_backward_wide_partials(int(R), int(H)))


def rnn_tanh_backward_step(dh_in, h_t, dhead, w_heads, a2, dz, dh_out, dbias_partials, out_scale=None, accumulate=False):
    """ic3_rnn_tanh_backward_step_wide: one step of the tanh recurrence's chain — dz = (dh_in + dhead . w_heads) * (1 - h_t^2),
    dh_out = (dz . a2) * out_scale, column sums of dz into dbias_partials (rnn_backward_partials(R, H) rows).  dh_in None: zeros;
    dh_out may be dh_in."""
    _need_cuda(h_t, "rnn_tanh_backward_step")
    R, H = h_t.shape
    OT = dhead.shape[-1]
    assert _f32(h_t, (R, H)) and _f32(dz, (R, H)) and _f32(dh_out, (R, H)) and _f32(dh_in, (R, H), none_ok=True)
    assert _f32(dhead, (R, OT))
    assert _dense(w_heads, (OT, H)) and _dense(a2, (H, H))
    assert _dense(dbias_partials, (rnn_backward_partials(R, H), H))
    return check(_lib.lib().ic3_rnn_tanh_backward_step_wide(ptr(dh_in), ptr(h_t), ptr(dhead), ptr(w_heads), OT, ptr(a2),
                                                            _rowvec(out_scale, R), ptr(dz), ptr(dh_out), ptr(dbias_partials),
                                                            int(bool(accumulate)), R, H, stream()))


def rnn_weight_grad(dz, h_prev, dA2, row_live=None, accumulate=True, work=None):
    """ic3_rnn_weight_grad_wide: dA2 (H, H) (+)= dz^T @ (row_live h_prev) over all Q rows of a window in one launch.  dz, h_prev (Q, H)
    contiguous (leading dims may be (T, R)), row_live (Q,) or None."""
    _need_cuda(dz, "rnn_weight_grad")
    H = dz.shape[-1]
    Q = dz.numel() // H
    assert _f32(dz) and _f32(h_prev) and h_prev.numel() >= Q * H and h_prev.shape[-1] == H
    assert _dense(dA2, (H, H))
    assert _f32(row_live, Q, none_ok=True)
    n = int(_lib.lib().ic3_rnn_weight_grad_wide_scratch_floats(Q, H))
    if n == 0:
        raise NotImplementedError("rnn_weight_grad: hid_size 64 / 128 / 256")
    check(_lib.lib().ic3_rnn_weight_grad_wide(ptr(dz), ptr(h_prev), ptr(row_live), Q, H, ptr(dA2), int(bool(accumulate)),
                                              ptr(_scratch(work, 'rnn_wgrad', n, dz.device)), stream()))


def rnn_backward(env, T, E, N, H, hs, dhead, snaps, a2, w_heads, dh, dz, dbias_partials, h_last=None, detach_gap=0, row_live=None,
                 row_keep=None, enc_first=True, enc_window=True, a2_grad=None, work=None, walk=False):
    """ic3_rnn_backward_wide: the backward through a window of T recorded steps of the tanh-recurrence baseline as one host call (one
    launch per step, the encoder's first stage over the dz ring — enc_window — or per step, and with a2_grad affine2's weight
    gradient over the window).  hs (>= T, R, H) the states entering the steps (slot T, or h_last, the state leaving the last one),
    dhead (T, R, OT), dz (T, R, H) the ring, dbias_partials (rnn_backward_partials(R, H), H) added to.
    walk: the T steps in ONE launch (an ic3_rnn_bptt_walk descriptor: every 64-row tile walked last step to first by one workgroup,
    dL/dh on chip) — the same dz, dh and a2_grad bit for bit; dbias_partials (ceil(R / 64), H), one row per tile."""
    _need_cuda(hs, "rnn_backward")
    R = E * N
    assert _f32(hs) and tuple(hs.shape[1:]) == (R, H)
    assert hs.shape[0] >= T + 1 or (hs.shape[0] >= T and h_last is not None)
    assert _dense(h_last, (R, H), none_ok=True)
    OT = _window_inputs(dhead, snaps, T, R)
    assert _dense(dh, (R, H)) and _dense(dz, (T, R, H))
    assert _dense(a2, (H, H)) and _dense(w_heads, (OT, H))
    assert _dense(dbias_partials, ((R + 63) // 64 if walk else rnn_backward_partials(R, H), H))
    assert _f32(row_live, (T, R), none_ok=True) and _f32(row_keep, (T, R), none_ok=True)
    b = (_lib.RnnBpttWalk if walk else _lib.RnnBptt)(T, E, N, H, OT, int(detach_gap), int(bool(enc_first)), int(bool(enc_window)))
    _set_ptrs(b, dict(hs=hs, dhead=dhead, snaps=snaps, a2=a2, w_heads=w_heads, dh=dh, dz=dz, dbias_partials=dbias_partials),
              h_last=h_last, row_live=row_live, row_keep=row_keep)
    b.snap_words = snaps.stride(0)
    b.enc_work = _enc_work(env, H, enc_window)
    scratch = _a2_grad_fill(b, a2_grad, work, T * R, H, hs.device)       # (`scratch`: alive until the call has returned)
    check(_lib.lib().ic3_rnn_backward_wide(env._h, C.byref(b), stream()))      # (its magic says which descriptor this is)


def mlp_backward_supported(env, H):
    """ic3_mlp_backward_wide_supported: the IC baseline's (models.MLP) window backward runs for this env handle at hid_size H."""
    return bool(_lib.lib().ic3_mlp_backward_wide_supported(env._h, int(H)))


def mlp_backward_partials(Q, H):
    """Rows of ic3_mlp_bptt.dbias_partials for a window of Q = T x R rows (ic3_mlp_backward_wide_partials)."""
    return int(_lib.lib().ic3_mlp_backward_wide_partials(int(Q), int(H)))


def mlp_backward_step(x1, h, dhead, w_heads, a2, dz, de, dbias_partials, accumulate=False):
    """ic3_mlp_backward_step_wide: the IC baseline's backward over Q independent rows in one launch — x1 (Q, H) holds e = affine1(obs)
    on entry and tanh(e) on return, dz = (dhead . w_heads) * (1 - h^2), de = (dz . a2 + dz) * (1 - x1^2), column sums of dz into
    dbias_partials (mlp_backward_partials(Q, H) rows).  Leading dims may be (T, R)."""
    _need_cuda(h, "mlp_backward_step")
    H = h.shape[-1]
    Q = h.numel() // H
    OT = dhead.shape[-1]
    for v in (x1, h, dz, de):
        assert _f32(v, Q * H) and v.shape[-1] == H
    assert _f32(dhead, Q * OT)
    assert _dense(w_heads, (OT, H)) and _dense(a2, (H, H))
    assert _dense(dbias_partials, (mlp_backward_partials(Q, H), H))
    return check(_lib.lib().ic3_mlp_backward_step_wide(ptr(x1), ptr(h), ptr(dhead), ptr(w_heads), OT, ptr(a2), ptr(dz), ptr(de),
                                                       ptr(dbias_partials), int(bool(accumulate)), Q, H, stream()))


def mlp_backward(env, T, E, N, H, h, dhead, snaps, enc_wt, enc_bias, a2, w_heads, x1, dz, de, dbias_partials, loc_table=None,
                 enc_first=True, enc_window=True, a2_grad=None, work=None):
    """ic3_mlp_backward_wide: the backward through a window of T recorded steps of the IC baseline (models.MLP) as one host call —
    T encoder launches into the x1 ring, ONE launch over all T x R rows, the encoder's first stage over the de ring (enc_window,
    or per step) and with a2_grad affine2's weight gradient over the window.  h (>= T, R, H) the state every step ended with,
    dhead (T, R, OT), x1 / dz / de (T, R, H) the rings, dbias_partials (mlp_backward_partials(T * R, H), H) written."""
    _need_cuda(h, "mlp_backward")
    R = E * N
    assert _f32(h) and tuple(h.shape[1:]) == (R, H) and h.shape[0] >= T
    OT = _window_inputs(dhead, snaps, T, R)
    assert _f32(x1, (T, R, H)) and _f32(dz, (T, R, H)) and _f32(de, (T, R, H))
    assert _f32(enc_wt, (env.obs_dim, H))
    assert _dense(enc_bias, H)
    assert _dense(a2, (H, H)) and _dense(w_heads, (OT, H))
    assert _dense(dbias_partials, (mlp_backward_partials(T * R, H), H))
    b = _lib.MlpBptt(T, E, N, H, OT, int(bool(enc_first)), int(bool(enc_window)))
    _set_ptrs(b, dict(h=h, dhead=dhead, snaps=snaps, enc_wt=enc_wt, enc_bias=enc_bias, a2=a2, w_heads=w_heads, x1=x1, dz=dz, de=de,
                      dbias_partials=dbias_partials), loc_table=loc_table)
    b.snap_words = snaps.stride(0)
    b.enc_work = _enc_work(env, H, enc_window)
    scratch = _a2_grad_fill(b, a2_grad, work, T * R, H, h.device)        # (`scratch`: alive until the call has returned)
    check(_lib.lib().ic3_mlp_backward_wide(env._h, C.byref(b), stream()))


def commnet_backward_supported(env, H, N):
    """ic3_commnet_backward_supported: the non-recurrent CommNet module's window backward runs for this env handle at hid_size H."""
    return bool(_lib.lib().ic3_commnet_backward_supported(env._h, int(H), int(N)))


def commnet_backward_chunk_steps(env, T, H, max_chunk_steps=0):
    """Steps per chunk of an ic3_commnet_backward window of T steps — what its rings are sized for (0: the call cannot run)."""
    return int(_lib.lib().ic3_commnet_backward_chunk_steps(env._h, int(T), int(H), int(max_chunk_steps)))


def commnet_backward_ring_floats(env, T, E, N, H, P, max_chunk_steps=0):
    """Floats of the rings + scratch ops.commnet_backward allocates for a window: with Qc = chunk steps x E x N rows, the enc /
    h_pass ring (P + 1) Qc H, dxh Qc 2H, dz, dx, de, dh Qc H each — (P + 7) Qc H — and ic3_commnet_backward_scratch_floats."""
    tc = commnet_backward_chunk_steps(env, T, H, max_chunk_steps)
    return (P + 7) * tc * E * N * H + int(_lib.lib().ic3_commnet_backward_scratch_floats(env._h, int(T), int(H), int(max_chunk_steps)))


def commnet_pass_backward_partials(Q, H):
    return int(_lib.lib().ic3_commnet_pass_backward_partials(int(Q), int(H)))


def commnet_pass_backward(dh_in, h_next, dhead, w_heads, f_weight, dxh, dz, dx, dbias_partials, dx_add=False, accumulate=False):
    """ic3_commnet_pass_backward: one communication pass of the module's backward over Q independent rows in one launch —
    dz = (dh_in + dhead . w_heads) * (1 - h_next^2) (either addend may be None) -> dz (Q, H) and dxh[:, :H]; dz . f_weight ->
    dxh[:, H:]; dx = dz or (dx_add) dx += dz; column sums of dz into dbias_partials (commnet_pass_backward_partials(Q, H) rows)."""
    _need_cuda(h_next, "commnet_pass_backward")
    Q, H = h_next.shape
    for v in (dh_in, h_next, dz, dx):
        assert _f32(v, (Q, H), none_ok=True)
    assert _f32(dxh, (Q, 2 * H))
    OT = 0
    if dhead is not None:
        OT = dhead.shape[-1]
        assert _f32(dhead, (Q, OT))
        assert _f32(w_heads, (OT, H))
    assert _f32(f_weight, (H, H))
    assert _dense(dbias_partials, (commnet_pass_backward_partials(Q, H), H))
    w_heads = w_heads if dhead is not None else None               # (dhead's weights: NULL without it)
    return check(_lib.lib().ic3_commnet_pass_backward(ptr(dh_in), ptr(h_next), ptr(dhead), ptr(w_heads), OT, ptr(f_weight), ptr(dxh),
                                                      ptr(dz), ptr(dx), int(bool(dx_add)), ptr(dbias_partials), int(bool(accumulate)),
                                                      Q, H, stream()))


def commnet_forward_record(enc, E, N, wp, bias, mode_avg, comm_zero, alive_in, comm_in, h_pass, wp3=None):
    """ic3_commnet_forward_record without the heads: h_pass (P + 1, E * N, H) <- h_0 = tanh(enc) .. h_P of every row; enc (E * N, H)
    may be h_pass[0] itself."""
    _need_cuda(enc, "commnet_forward_record")
    R, H = enc.shape
    P = wp.shape[0]
    assert R == E * N and _f32(enc)
    assert _f32(h_pass, (P + 1, R, H))
    assert _mask(alive_in, R) and _mask(comm_in, R)
    assert _dense(wp3, (P, 3 * H * H), none_ok=True)
    check(_lib.lib().ic3_commnet_forward_record(ptr(enc), E, N, H, P, ptr(wp), ptr(wp3), ptr(bias), None, None, None, 0,
                                                int(bool(mode_avg)), int(bool(comm_zero)), ptr(alive_in), ptr(comm_in), None, None,
                                                ptr(h_pass), stream()))
    return h_pass


def commnet_backward(env, T, E, N, H, dhead, snaps, alive, gate, enc_wt, enc_bias, wp, bias, w_heads, f_weights, c_weights, f_grads,
                     c_grads, bias_grads, heads_w_grad=None, heads_b_grad=None, wp3=None, loc_table=None, mode_avg=True, comm_zero=False,
                     enc_first=True, enc_window=True, max_chunk_steps=0, work=None):
    """ic3_commnet_backward: the backward through a window of T recorded steps of the non-recurrent CommNet module as one host call
    (csrc/bptt_kernels.hip) — T encoder launches, the recording forward over T x E envs, per pass the pass launch, ic3_comm_backward
    and the weight gradient over all rows, the pointwise step through x, the encoder's first stage, the heads' gradient.  dhead
    (T, R, OT), alive / gate (T, E, N) int32 or None, f_weights / c_weights: lists of P (H, H) weights as stored, f_grads / c_grads
    (H, H) / bias_grads (H,): lists of P DISTINCT tensors, added to; heads_w_grad (OT, H) / heads_b_grad (OT,) added to.  The rings
    (commnet_backward_ring_floats) live in `work` between calls.  Returns (rings dict, chunks run)."""
    _need_cuda(dhead, "commnet_backward")
    R, P = E * N, len(f_weights)
    dev = dhead.device
    OT = _window_inputs(dhead, snaps, T, R)
    assert _i32(alive, (T, E, N), none_ok=True) and _i32(gate, (T, E, N), none_ok=True)
    assert _f32(enc_wt, (env.obs_dim, H))
    assert _dense(enc_bias, H)
    assert _dense(wp, (P, 2 * H * H)) and _dense(bias, (P, H))
    assert _dense(wp3, (P, 3 * H * H), none_ok=True)
    assert _dense(w_heads, (OT, H))
    mats = list(f_weights) + list(f_grads) + ([] if comm_zero else list(c_weights) + list(c_grads))
    assert len(f_grads) == len(bias_grads) == P and (comm_zero or len(c_weights) == len(c_grads) == P)
    assert all(_f32(v, (H, H)) for v in mats)
    assert all(_f32(v, H) for v in bias_grads)
    assert len(set(v.data_ptr() for v in f_grads)) == P and len(set(v.data_ptr() for v in bias_grads)) == P
    tc = commnet_backward_chunk_steps(env, T, H, max_chunk_steps)
    if tc < 1:
        raise NotImplementedError("commnet_backward: hid_size %d / this window cannot run" % H)
    Qc = tc * R
    nscr = int(_lib.lib().ic3_commnet_backward_scratch_floats(env._h, T, H, int(max_chunk_steps)))
    buf = _scratch(work, 'commnet_bwd', (P + 7) * Qc * H + nscr, dev)
    off = [0]

    def take(*shape):
        n = 1
        for s in shape:
            n *= s
        v = buf[off[0]:off[0] + n].view(*shape)
        off[0] += n
        return v
    rings = dict(h_pass=take(P + 1, Qc, H), dxh=take(Qc, 2 * H), dz=take(Qc, H), dx=take(Qc, H), de=take(Qc, H), dh=take(Qc, H))
    scratch = take(nscr)
    arr = lambda lst: (C.c_void_p * P)(*[v.data_ptr() for v in lst])
    b = _lib.CommnetBptt(T, E, N, H, OT, P, int(bool(mode_avg)), int(bool(comm_zero)), int(bool(enc_first)), int(bool(enc_window)),
                         int(max_chunk_steps))
    _set_ptrs(b, dict(rings, dhead=dhead, snaps=snaps, enc_wt=enc_wt, enc_bias=enc_bias, wp=wp, bias=bias, w_heads=w_heads,
                      scratch=scratch), alive=alive, gate=gate, loc_table=loc_table, wp3=wp3)
    b.snap_words = snaps.stride(0)
    keep = [arr(f_weights), arr(f_grads), arr(bias_grads)]      # (alive until the call has returned)
    b.f_weight, b.f_grad, b.bias_grad = keep
    if not comm_zero:
        keep += [arr(c_weights), arr(c_grads)]
        b.c_weight, b.c_grad = keep[3:]
    if heads_w_grad is not None:
        assert _dense(heads_w_grad, (OT, H)) and _dense(heads_b_grad, OT)
        _set_ptrs(b, dict(heads_w_grad=heads_w_grad, heads_b_grad=heads_b_grad))
    b.enc_work = _enc_work(env, H, enc_window)
    chunks = check(_lib.lib().ic3_commnet_backward(env._h, C.byref(b), stream()))
    return rings, chunks


HEADS_GRAD_MAX_OT = 16      # ic3_heads_grad: at most 16 output columns (the heads' actions in total + the value)


def heads_grad(d, h, dW, db, work=None):
    """dW (OT,H) += d^T . h, db (OT,) += column sums of d over all M rows of d (M,OT) / h (M,H) — ic3_heads_grad: the heads'
    weight gradient of a whole episode in one pass."""
    _need_cuda(d, "heads_grad")
    M, OT = d.shape
    H = h.shape[1]
    assert _f32(d) and _f32(h) and h.shape[0] == M
    assert _dense(dW, (OT, H)) and _dense(db, OT)
    scratch = _scratch(work, ('heads_grad', H), int(_lib.lib().ic3_heads_grad_scratch_floats(H)), d.device)
    check(_lib.lib().ic3_heads_grad(ptr(d), ptr(h), M, H, OT, ptr(dW), ptr(db), ptr(scratch), stream()))


def policy_heads(h, W, b, head_sizes, out=None):
    """h (R,H) rows (unit column stride), W (OT,H), b (OT,) -> out (R,OT) = [log_softmax heads | value]."""
    _need_cuda(h, "policy_heads")
    R, H = h.shape
    OT = W.shape[0]
    assert h.stride(1) == 1 and _dense(W) and OT == sum(head_sizes) + 1
    if out is None:
        out = torch.empty((R, OT), dtype=torch.float32, device=h.device)
    sizes = int32_array(head_sizes)
    check(_lib.lib().ic3_policy_heads(ptr(h), h.stride(0), ptr(W), ptr(b), sizes, len(head_sizes), ptr(out), R, H,
                                      stream()))
    return out


POLICY_STEP_SIZES = (64, 128, 256)


def padded_hidden(H):
    """The next hidden size the one-launch kernels are built for, or None (H is one of them, or larger than all):
    comm.CommNetMLP runs other sizes zero-padded to it (exact: a padded unit's pre-activations, state and output are 0)."""
    H = int(H)
    if H in POLICY_STEP_SIZES or H < 1:
        return None
    for s in POLICY_STEP_SIZES:
        if H < s:
            return s
    return None


def policy_step_pack(c_weight, w_ih, w_hh):
    """C.weight (H,H) and [W_ih | W_hh] (4H, 2H) in the layout ic3_policy_step streams (ic3_policy_pack)."""
    _need_cuda(c_weight, "policy_step_pack")
    H = c_weight.shape[0]
    dev = c_weight.device
    c_wp = torch.empty((H * H,), dtype=torch.float32, device=dev)
    l_wp = torch.empty((8 * H * H,), dtype=torch.float32, device=dev)
    check(_lib.lib().ic3_policy_pack(ptr(c_weight.detach().contiguous().float()), ptr(w_ih.detach().contiguous().float()),
                                     ptr(w_hh.detach().contiguous().float()), ptr(c_wp), ptr(l_wp), H, stream()))
    return dict(ps_c_wp=c_wp, ps_l_wp=l_wp)


def policy_step_supported(env, H):
    """True when ic3_policy_step can run this env / hid_size (env: the raw batched env object)."""
    return H in POLICY_STEP_SIZES and _lib.lib().ic3_policy_step_supported(env._h, int(H)) > 0


def _pack_split(entry, name, w_ih, w_hh):
    """[W_ih | W_hh] (4H, 2H) as three bf16 planes (24 H^2 words) in the fragment order `entry` writes."""
    _need_cuda(w_ih, name)
    H = w_ih.shape[1]
    wp3 = torch.empty((3 * 2 * H * 4 * H,), dtype=torch.bfloat16, device=w_ih.device)
    check(entry(ptr(w_ih.detach().contiguous().float()), ptr(w_hh.detach().contiguous().float()), ptr(wp3), H, stream()))
    return wp3


def policy_pack_split(w_ih, w_hh):
    """ic3_policy.gate_split (the default): [W_ih | W_hh] as three exact bf16 planes in MFMA fragment order."""
    return _pack_split(_lib.lib().ic3_policy_pack_split, "policy_pack_split", w_ih, w_hh)


def policy_pack_split_bwd(w_ih, w_hh):
    """The split planes of [W_ih | W_hh] in the fragment order of the gate product's BACKWARD (ic3_lstm_gates_backward_dx)."""
    return _pack_split(_lib.lib().ic3_policy_pack_split_bwd, "policy_pack_split_bwd", w_ih, w_hh)


def policy_step_passes_supported(fc, H, passes, wide_passes=False):
    """comm_passes > 1 as a loop INSIDE one ic3_policy_step launch (ic3_policy.npasses): the split gate product, hid 64 / 128,
    at most 4 passes; otherwise one launch per pass.  wide_passes: hid 256 as well (the library runs it there; this layer asks for
    it only behind --passes_in_launch_wide)."""
    return 2 <= passes <= 4 and (H in (64, 128) or (bool(wide_passes) and H == 256)) and fc.get('ps_l_wp3') is not None


def _policy_struct(fc, H, head_sizes, mode_avg, comm_zero, encoder=True, pass_index=0, inner=False, passes=1):
    """pass_index / inner: comm_passes > 1 — pass i uses C_modules[i] (cache keys '<name>_p<i>' for i > 0), every pass but
    the last is an `inner` one (h, c only).  passes >= 2: all of them in one launch (npasses)."""
    sfx = '' if pass_index == 0 else '_p%d' % pass_index
    pol = _lib.Policy()
    pol.pass_index, pol.inner_pass = int(pass_index), int(bool(inner))
    if passes >= 2:
        assert pass_index == 0 and not inner and encoder
        pol.npasses = int(passes)
        for i in range(passes):
            sf = '' if i == 0 else '_p%d' % i
            pol.c_wp_pass[i] = fc['ps_c_wp' + sf].data_ptr()
            pol.enc_bias_pass[i] = fc['enc_bias' + sf].data_ptr()
    pol.H, pol.nheads = int(H), len(head_sizes)
    pol.head_sizes = int32_array(head_sizes, 4)
    pol.mode_avg, pol.comm_zero = int(bool(mode_avg)), int(bool(comm_zero))
    if encoder:
        _set_ptrs(pol, dict(enc_wt=fc['wt'], enc_bias=fc['enc_bias' + sfx]), loc_table=fc.get('loc_table'))
    _set_ptrs(pol, dict(c_wp=fc['ps_c_wp' + sfx], lstm_wp=fc['ps_l_wp'], lstm_bias=fc['b_cat'], head_w=fc['w_heads'],
                        head_b=fc['b_heads']), lstm_wp3=fc.get('ps_l_wp3'))
    pol.gate_split = int(fc.get('ps_l_wp3') is not None)         # exact split products on the bf16 matrix cores
    return pol


def policy_forward(fc, H, head_sizes, mode_avg, comm_zero, enc, E, N, h, c, alive_in, comm_in, out=None, pass_index=0,
                   inner=False):
    """The policy half of policy_step for a caller-supplied encoder output enc (E*N, H) = encoder(x) + C.bias
    (ic3_policy_forward): communication block, C, LSTMCell, heads, log_softmax in one launch; h, c in place.
    inner=True: a non-final communication pass (comm_passes > 1) — h, c only, returns None."""
    _need_cuda(enc, "policy_forward")
    R = E * N
    assert _dense(enc, (R, H)) and _dense(h) and _dense(c)
    assert _mask(alive_in, R) and _mask(comm_in, R)
    if out is None and not inner:
        out = torch.empty((R, sum(head_sizes) + 1), dtype=torch.float32, device=enc.device)
    pol = _policy_struct(fc, H, head_sizes, mode_avg, comm_zero, encoder=False, pass_index=pass_index, inner=inner)
    check(_lib.lib().ic3_policy_forward(C.byref(pol), ptr(enc), E, N, ptr(h), ptr(c), ptr(alive_in), ptr(comm_in),
                                        None if inner else ptr(out), stream()))
    return None if inner else out


def policy_forward_record(fc, H, head_sizes, mode_avg, comm_zero, enc, E, N, h_in, c_in, h_out, c_out, alive_in, comm_in, gates, inp,
                          pass_index=0, enc_add=None):
    """ic3_policy_forward on an ic3_policy_record: communication pass `pass_index` of a comm_passes > 1 step as a recording inner pass over E envs (a
    chunk of whole steps: Tc x E envs, masks stacked) — (h_in, c_in) -> (h_out, c_out) (E*N, H), the activated gates (E*N, 4H) and the
    inp rows (E*N, record_xh_width(H)); enc (E*N, H) = encoder(x) + encoder.bias + C_0.bias, enc_add (H,) = C_i.bias - C_0.bias or
    None.  Needs the split planes (fc['ps_l_wp3'])."""
    _need_cuda(enc, "policy_forward_record")
    R = E * N
    assert _dense(enc, (R, H)) and _f32(enc_add, H, none_ok=True)
    assert _dense(h_in, (R, H)) and _dense(c_in, (R, H)) and _dense(h_out, (R, H)) and _dense(c_out, (R, H))
    assert _dense(gates, (R, 4 * H)) and _dense(inp, (R, record_xh_width(H)))
    assert _mask(alive_in, R) and _mask(comm_in, R)
    pol = _policy_struct(fc, H, head_sizes, mode_avg, comm_zero, encoder=False, pass_index=pass_index, inner=True)
    rec = _lib.PolicyRecord()
    C.memmove(C.addressof(rec), C.addressof(pol), C.sizeof(pol))
    rec.struct_size, rec.inner_pass = C.sizeof(rec), rec.RECORD_PASS
    _set_ptrs(rec, dict(h_out=h_out, c_out=c_out, gates=gates, inp=inp), enc_add=enc_add)
    check(_lib.lib().ic3_policy_forward(C.cast(C.byref(rec), C.POINTER(_lib.Policy)), ptr(enc), E, N, ptr(h_in), ptr(c_in), ptr(alive_in),
                                        ptr(comm_in), None, stream()))


def policy_step_pass(env, fc, H, head_sizes, mode_avg, comm_zero, h, c, alive_in, comm_in, pass_index):
    """A non-final communication pass of a comm_passes > 1 policy on the env's own state (ic3_policy_step with
    ic3_policy.inner_pass): sparse encoder, communication block, C_modules[pass_index], LSTMCell — h, c in place."""
    _need_cuda(h, "policy_step_pass")
    pol = _policy_struct(fc, H, head_sizes, mode_avg, comm_zero, pass_index=pass_index, inner=True)
    check(_lib.lib().ic3_policy_step(env._h, C.byref(pol), ptr(h), ptr(c), ptr(alive_in), ptr(comm_in), None, None, None,
                                     None, None, None, None, stream()))


def policy_step(env, fc, H, head_sizes, mode_avg, comm_zero, h, c, alive_in, comm_in, out, action, reward, done,
                alive=None, is_completed=None, obs=None, pass_index=0, passes=1):
    """One whole rollout iteration (policy forward -> action draws -> env.step) in one launch — ic3_policy_step.
    `fc`: the policy's derived-weight cache (wt, enc_bias, loc_table, ps_c_wp, ps_l_wp, b_cat, w_heads, b_heads);
    h, c (E*N, H) contiguous, updated in place; out (E*N, OT); action (heads, E, N) int32."""
    _need_cuda(h, "policy_step")
    R = h.shape[0]
    assert _dense(h, (R, H)) and _dense(c, (R, H))
    assert _dense(out, (R, sum(head_sizes) + 1)) and _i32(action, len(head_sizes) * R)
    assert _mask(alive_in, R) and _mask(comm_in, R)
    pol = _policy_struct(fc, H, head_sizes, mode_avg, comm_zero, pass_index=pass_index, passes=passes)
    check(_lib.lib().ic3_policy_step(env._h, C.byref(pol), ptr(h), ptr(c), ptr(alive_in), ptr(comm_in), ptr(out),
                                     ptr(action), ptr(obs), ptr(reward), ptr(done), ptr(alive), ptr(is_completed), stream()))
    return out


WINDOW_COMM_MODES = dict(all=_lib.PolicyWindow.COMM_ALL, last_head=_lib.PolicyWindow.COMM_LAST_HEAD, ones=_lib.PolicyWindow.COMM_ONES)


def policy_step_window_supported(env, fc, H, passes=1, wide=False, wide_passes=False, record_passes=False):
    """ic3_policy_step on an ic3_policy_window can run this env / hid_size: the split gate product, hid 64 / 128, a tile that fits;
    passes 2..4: the form tagged WINDOW_PASSES, where the per-step call would be the in-launch pass loop.  wide: the form tagged
    WINDOW_WIDE — hid 256 and one pass, nothing else (hid 64 / 128 are the narrow tag's).  wide_passes: the form tagged
    WINDOW_WIDE_PASSES — hid 256 and passes 2..4, nothing else (every other shape is answered as without it).  record_passes: the
    form tagged WINDOW_PASSES_RECORD — hid 64 / 128 and passes 2..4, nothing else."""
    if record_passes:
        return H in (64, 128) and 2 <= int(passes) <= 4 and fc.get('ps_l_wp3') is not None and \
            policy_step_passes_supported(fc, H, passes) and policy_step_supported(env, H)
    if wide_passes and H == 256 and passes != 1:
        return policy_step_passes_supported(fc, H, passes, wide_passes=True) and policy_step_supported(env, H)
    if passes != 1 and not policy_step_passes_supported(fc, H, passes):
        return False
    if wide:
        return H == 256 and passes == 1 and fc.get('ps_l_wp3') is not None and policy_step_supported(env, H)
    return H in (64, 128) and fc.get('ps_l_wp3') is not None and policy_step_supported(env, H)


def policy_step_window(env, fc, H, head_sizes, mode_avg, comm_zero, T, hs, cs, alive_in, comm_in, out, action, reward, done,
                       alive=None, is_completed=None, gates=None, inp=None, snaps=None, alive_prev=False, comm_mode='all', passes=1,
                       wide=False, wide_passes=False, record_passes=None):
    """T consecutive policy_step calls of the recorded training rollout in ONE launch — ic3_policy_step on an ic3_policy_window.
    hs, cs (T+1, E*N, H): step t reads slot t and writes slot t+1; alive_in / comm_in: the masks of step 0; out (T, E*N, OT); action
    (T, heads, E, N) int32; reward / alive / is_completed (T, E, N); done (T, E); gates (T, E*N, 4H) with inp (T, E*N, 2H) or both
    None; snaps (T, words >= state_words) int32 or None: the env state entering every step.  The masks of step t >= 1: alive_prev —
    the alive slice of step t-1 (Traffic-Junction), else everyone; comm_mode 'all' | 'last_head' (the last head's draws of step t-1)
    | 'ones'.  No dense observation rows.  Same bits as T policy_step calls on the same handle.  passes >= 2: every step runs that
    many communication passes inside the launch (the descriptor tagged WINDOW_PASSES, the passes' weights from `fc` as policy_step
    takes them); no gate record then.  wide: the descriptor tagged WINDOW_WIDE — hid 256, one pass, and inp (T, E*N, H): the inp rows
    alone (record_xh_width).  wide_passes: the descriptor tagged WINDOW_WIDE_PASSES — hid 256, passes 2..4, no gate record.
    record_passes: dict(gates=, inp=, h=, c=) — the descriptor tagged WINDOW_PASSES_RECORD (hid 64 / 128, passes 2..4): the same
    window, which also stores pass i's activated gates to gates[i] (T, E*N, 4H), its inp rows to inp[i] (T, E*N, 2H) (the inp half)
    and, for i >= 1, the (h, c) entering pass i to h[i] / c[i] (T, E*N, H); every argument is indexable by the pass, entries 0 of h
    and c are not read.
    NotImplementedError where the library answers -ENOSYS."""
    _need_cuda(hs, "policy_step_window")
    T = int(T)
    R, nh, OT = hs.shape[1], len(head_sizes), sum(head_sizes) + 1
    assert T >= 1 and _dense(hs, (T + 1, R, H)) and _dense(cs, (T + 1, R, H))
    assert _dense(out, (T, R, OT)) and _i32(action, T * nh * R)
    assert _mask(alive_in, R) and _mask(comm_in, R)
    assert _f32(reward, T * R) and _i32(alive, T * R, none_ok=True) and _i32(is_completed, T * R, none_ok=True)
    assert _i32(done, T * env.nenvs)
    assert not wide or (H == 256 and int(passes) == 1), "WINDOW_WIDE is the one-pass window at hid 256"
    assert not wide_passes or (H == 256 and 2 <= int(passes) <= 4 and not wide), "WINDOW_WIDE_PASSES is the 2..4-pass window at hid 256"
    XW = record_xh_width(H) if wide else 2 * H
    assert (gates is None) == (inp is None) and (gates is None or (_dense(gates, (T, R, 4 * H)) and _dense(inp, (T, R, XW))))
    assert snaps is None or (snaps.dtype == torch.int32 and snaps.is_contiguous() and snaps.dim() == 2 and snaps.shape[0] == T)
    assert not alive_prev or alive is not None
    passes = int(passes)
    assert passes == 1 or gates is None, "the in-launch passes keep no gate record"
    pol = _policy_struct(fc, H, head_sizes, mode_avg, comm_zero, passes=passes)
    win = _lib.PolicyWindow() if record_passes is None else _lib.PolicyWindowRecord()
    C.memmove(C.addressof(win), C.addressof(pol), C.sizeof(pol))
    PW = _lib.PolicyWindow
    win.struct_size, win.inner_pass = C.sizeof(win), PW.WINDOW_WIDE_PASSES if wide_passes else PW.WINDOW_WIDE if wide else \
        PW.WINDOW if passes == 1 else PW.WINDOW_PASSES
    win.T = T
    win.alive_mode = PW.ALIVE_PREV if alive_prev else PW.ALIVE_ALL
    win.comm_mode = WINDOW_COMM_MODES[comm_mode]
    _set_ptrs(win, dict(), gates=gates, inp=inp, snaps=snaps)
    win.snap_words = int(snaps.shape[1]) if snaps is not None else 0
    if record_passes is not None:
        assert H in (64, 128) and 2 <= passes <= 4 and not wide and not wide_passes, "WINDOW_PASSES_RECORD is the 2..4-pass window at hid 64 / 128"
        win.inner_pass = win.WINDOW_PASSES_RECORD
        for i in range(passes):
            assert _dense(record_passes['gates'][i], (T, R, 4 * H)) and _dense(record_passes['inp'][i], (T, R, 2 * H))
            win.gates_pass[i], win.inp_pass[i] = record_passes['gates'][i].data_ptr(), record_passes['inp'][i].data_ptr()
            if i >= 1:
                assert _dense(record_passes['h'][i], (T, R, H)) and _dense(record_passes['c'][i], (T, R, H))
                win.h_pass[i], win.c_pass[i] = record_passes['h'][i].data_ptr(), record_passes['c'][i].data_ptr()
    check(_lib.lib().ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(_lib.Policy)), ptr(hs), ptr(cs), ptr(alive_in),
                                     ptr(comm_in), ptr(out), ptr(action), None, ptr(reward), ptr(done), ptr(alive),
                                     ptr(is_completed), stream()))
    return out


def commnet_step_window_supported(env, cn, H, wide=False):
    """ic3_policy_step on an ic3_commnet_window can run this env / hid_size: the split products, hid 64 / 128, a tile that fits.
    wide: the form tagged WINDOW_WIDE — hid 256, nothing else."""
    return (H == 256 if wide else H in (64, 128)) and cn.get('wp3') is not None and commnet_step_supported(env, H)


def commnet_step_window(env, cn, H, head_sizes, mode_avg, comm_zero, T, alive_in, comm_in, out, action, reward, done, alive,
                        is_completed, hs=None, h_fin=None, snaps=None, alive_prev=False, comm_mode='all', wide=False):
    """T consecutive commnet_step calls of the recorded training rollout in ONE launch — ic3_policy_step on an ic3_commnet_window.
    `cn`: the module's derived weights, as for commnet_step.  alive_in / comm_in: the masks of step 0; out (T, E*N, OT); action
    (T, heads, E, N) int32; reward / alive / is_completed (T, E, N); done (T, E).  hs (T+1, E*N, H): the tanh recurrence — step t
    reads slot t as h_in and writes slot t+1 — or None; h_fin (T, E*N, H) or None: the module's final hidden state of every step;
    snaps (T, words >= state_words) int32 or None: the env state entering every step.  The masks of step t >= 1 as in
    policy_step_window.  No dense observation rows.  Same bits as T commnet_step calls.  wide: the descriptor tagged WINDOW_WIDE —
    hid 256.  NotImplementedError where the library answers -ENOSYS (hid 256 without `wide`, no split planes, a tile that does not
    fit)."""
    _need_cuda(out, "commnet_step_window")
    T, H = int(T), int(H)
    assert not wide or H == 256, "WINDOW_WIDE is the window at hid 256"
    R, nh, OT = out.shape[1], len(head_sizes), sum(int(a) for a in head_sizes) + 1
    assert T >= 1 and _dense(out, (T, R, OT), torch.float32) and _i32(action, T * nh * R)
    assert _mask(alive_in, R) and _mask(comm_in, R)
    assert _f32(reward, T * R) and _i32(alive, T * R, none_ok=True) and _i32(is_completed, T * R, none_ok=True)
    assert _i32(done, T * env.nenvs)
    assert _f32(hs, (T + 1, R, H), none_ok=True) and _f32(h_fin, (T, R, H), none_ok=True)
    assert snaps is None or (snaps.dtype == torch.int32 and snaps.is_contiguous() and snaps.dim() == 2 and snaps.shape[0] == T)
    assert not alive_prev or alive is not None
    win = _lib.CommnetWindow()
    win.inner_pass = win.WINDOW_WIDE if wide else win.WINDOW
    win.H, win.nheads, win.head_sizes = H, nh, int32_array(head_sizes, 4)
    win.mode_avg, win.comm_zero, win.npasses = int(bool(mode_avg)), int(bool(comm_zero)), int(cn['wp'].shape[0])
    win.T, win.recurrence = T, int(hs is not None)
    win.alive_mode = _lib.PolicyWindow.ALIVE_PREV if alive_prev else _lib.PolicyWindow.ALIVE_ALL
    win.comm_mode = WINDOW_COMM_MODES[comm_mode]
    _set_ptrs(win, dict(enc_wt=cn['wt'], enc_bias=cn['enc_bias'], head_w=cn['w_heads'], head_b=cn['b_heads'], wp=cn['wp'], bias=cn['bias']),
              loc_table=cn['loc_table'], wp3=cn.get('wp3'), h_fin=h_fin, snaps=snaps)
    win.snap_words = int(snaps.shape[1]) if snaps is not None else 0
    check(_lib.lib().ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(_lib.Policy)), ptr(hs), None, ptr(alive_in), ptr(comm_in),
                                     ptr(out), ptr(action), None, ptr(reward), ptr(done), ptr(alive), ptr(is_completed), stream()))
    return out


def episode_finalize(done, reward, alive=None, is_completed=None, gate=None, gate_ones=False, auto_reset=False,
                     forced_last=False, work=None):
    """The per-step derivations of get_episode (trainer.py:70-105,109-110) for n slots of E envs in one launch —
    ic3_episode_finalize.  done (n, E) int32; reward (n, E, N) f32; alive / is_completed (n, E, N) int32 or None;
    gate (n, E, N) int32 view with contiguous (E, N) slots (the talk head's actions) or None.
    Returns dict(live (n,E), alive_mask, episode_mask (n,E), episode_mini_mask, live_after (E,), stats) where `stats`
    is a device fp64 tensor [num_steps, zero_len_envs, reward_sum[N], gate_sum[N]] (read it after a sync).
    `work`: dict reused between calls for the scratch buffers."""
    _need_cuda(reward, "episode_finalize")
    n, E, N = reward.shape
    dev = reward.device
    assert _i32(done, (n, E))
    assert _f32(reward)
    assert _i32(alive, (n, E, N), none_ok=True) and _i32(is_completed, (n, E, N), none_ok=True)
    gate_stride = 0
    if gate is not None:
        assert gate.dtype == torch.int32 and gate.shape == (n, E, N) and gate[0].is_contiguous()
        gate_stride = gate.stride(0) if n > 1 else E * N
    work = work if work is not None else dict()
    key = (E, N, str(dev))
    if work.get('key') != key:
        nbytes = int(_lib.lib().ic3_episode_scratch_bytes(E, N))
        if nbytes == 0:
            raise ValueError("episode_finalize: unsupported sizes E=%d N=%d" % (E, N))
        work.update(key=key, scratch=torch.empty(nbytes // 8, dtype=torch.float64, device=dev),
                    counter=torch.zeros(1, dtype=torch.int32, device=dev))
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    res = dict(live=f(n, E), alive_mask=f(n, E, N), episode_mask=f(n, E), episode_mini_mask=f(n, E, N),
               live_after=f(E), stats=torch.empty(2 + 2 * N, dtype=torch.float64, device=dev))
    ep = _lib.Episode(n, E, N, int(bool(auto_reset)), int(bool(forced_last)), int(bool(gate_ones)), ptr(done),
                      ptr(alive), ptr(is_completed), ptr(reward), ptr(gate), gate_stride, ptr(res['live']),
                      ptr(res['alive_mask']), ptr(res['episode_mask']), ptr(res['episode_mini_mask']),
                      ptr(res['live_after']), ptr(res['stats']), ptr(work['scratch']), ptr(work['counter']))
    check(_lib.lib().ic3_episode_finalize(C.byref(ep), stream()))
    return res


def returns_scan(rewards, episode_masks, episode_mini_masks, gamma, mean_ratio):
    """trainer.py:162-171: returns (T, E, N) = mean_ratio * mean over agents of the cooperative returns + (1 - mean_ratio) *
    the per-agent returns, both scanned backwards over the T slots with episode_mask (and episode_mini_mask) cutting the
    recursion — ic3_returns_scan, one launch instead of ~9 tensor ops per slot.  episode_masks (T, E) or (T, E, N) expanded."""
    _need_cuda(rewards, "returns_scan")
    T, E, N = rewards.shape
    em = episode_masks[:, :, 0] if episode_masks.dim() == 3 else episode_masks
    rewards, em, mm = rewards.contiguous().float(), em.contiguous().float(), episode_mini_masks.contiguous().float()
    out = torch.empty_like(rewards)
    check(_lib.lib().ic3_returns_scan(ptr(rewards), ptr(em), ptr(mm), float(gamma), float(mean_ratio), ptr(out), T, E, N, stream()))
    return out


def loss_gradients(out, action, returns, alive_mask, live, head_sizes, entr, value_coeff, adv_shift=0.0, adv_scale=1.0):
    """compute_grad's losses and dL/d[logits | value] of every transition in one launch (ic3_loss_gradients): out (T, R, OT) the
    step launches' rows, action (T, heads, R) int32, returns / alive_mask (T, R), live (T, E).  Returns (d_out (T, R, OT),
    (action_loss, value_loss, entropy) as a float64 tensor of 3 on the device)."""
    _need_cuda(out, "loss_gradients")
    T, R, OT = out.shape
    E = live.shape[1]
    N = R // E
    nh = len(head_sizes)
    assert OT == sum(int(a) for a in head_sizes) + 1 and tuple(action.shape) == (T, nh, R) and action.dtype == torch.int32
    for v in (out, action, returns, alive_mask, live):
        assert _dense(v)
    assert returns.numel() == T * R == alive_mask.numel() and live.numel() == T * E and E * N == R
    d_out = torch.empty_like(out)
    sums = torch.empty((int(_lib.lib().ic3_loss_gradients_partials(T, R)), 3), dtype=torch.float64, device=out.device)
    sizes = int32_array(head_sizes)
    check(_lib.lib().ic3_loss_gradients(ptr(out), ptr(action), ptr(returns), ptr(alive_mask), ptr(live), sizes, nh,
                                        float(adv_shift), float(adv_scale), float(entr), float(value_coeff), ptr(d_out), ptr(sums),
                                        T, E, N, stream()))
    return d_out, sums.sum(0)


def lstm_cell_heads_ok(H):
    """ic3_lstm_cell_heads needs H/4 to be a power of two <= 64."""
    return H % 4 == 0 and H // 4 <= 64 and (H // 4) & (H // 4 - 1) == 0


def lstm_cell_heads_(gates, c, h_out, W, b, head_sizes, out=None, env=None, action=None):
    """lstm_cell_ + policy_heads (+ the action draws of every head into `action` (heads, E, N) int32 when `env`, the
    raw batched env, is given) in one launch.  Returns out (R, OT)."""
    _need_cuda(gates, "lstm_cell_heads_")
    R, H = c.shape
    OT = W.shape[0]
    assert _dense(gates) and _dense(c) and h_out.stride(1) == 1 and _dense(W)
    assert OT == sum(head_sizes) + 1
    if out is None:
        out = torch.empty((R, OT), dtype=torch.float32, device=c.device)
    if action is not None:
        assert env is not None and _i32(action, len(head_sizes) * R)
    sizes = int32_array(head_sizes)
    check(_lib.lib().ic3_lstm_cell_heads(ptr(gates), ptr(c), ptr(h_out), h_out.stride(0), R, H, ptr(W), ptr(b), sizes,
                                         len(head_sizes), ptr(out), env._h if action is not None else None, ptr(action),
                                         stream()))
    return out


def comm_masked_mean(h, alive=None, comm_action=None, mode_avg=True, mask_self=True):
    """h (E,N,H) f32; alive / comm_action (E,N) int32 CUDA tensors or None -> (E,N,H)."""
    if alive is not None:
        alive = alive.to(torch.int32).contiguous()
    if comm_action is not None:
        comm_action = comm_action.to(torch.int32).contiguous()
    return _CommMaskedMean.apply(h, alive, comm_action, mode_avg, mask_self)


def _draw_buffers(logp, out, want_logp):
    """(logp rows for the kernel, their stride, action (E,N) int32 = `out` or a new tensor, chosen log-prob (E,N) f32 or None)"""
    E, N, A = logp.shape
    logp, ld = _rows(logp.detach(), A)
    action = out if out is not None else torch.empty((E, N), dtype=torch.int32, device=logp.device)
    chosen = torch.empty((E, N), dtype=torch.float32, device=logp.device) if want_logp else None
    return logp, ld, action, chosen


def sample_actions(logp, head, seed, env_id_offset, episode, t, want_logp=False, out=None):
    """logp (E,N,A) f32 -> action (E,N) int32 [, chosen log-prob (E,N) f32]; action_utils.py:32-36."""
    _need_cuda(logp, "sample_actions")
    E, N, A = logp.shape
    logp, ld, action, chosen = _draw_buffers(logp, out, want_logp)
    check(_lib.lib().ic3_sample_actions(ptr(logp), ld, A, int(head), int(seed) & 0xffffffff, int(env_id_offset),
                                        int(episode), int(t), ptr(action), ptr(chosen), E, N, stream()))
    return (action, chosen) if want_logp else action


def sample_actions_env(env, logp, head, out=None, want_logp=False):
    """sample_actions with (seed, env_id_offset, episode, t) taken from the env handle's own device-side counters
    (ic3_env_sample_actions): identical draws, but every launch argument is constant -> hipGraph-capturable."""
    _need_cuda(logp, "sample_actions_env")
    E, N, A = logp.shape
    logp, ld, action, chosen = _draw_buffers(logp, out, want_logp)
    check(_lib.lib().ic3_env_sample_actions(env._h, ptr(logp), ld, A, int(head), ptr(action), ptr(chosen), stream()))
    return (action, chosen) if want_logp else action


def random_actions(E, N, naction, seed, env_id_offset, episode, t, device='cuda', out=None):
    action = out if out is not None else torch.empty((E, N), dtype=torch.int32, device=device)
    with torch.cuda.device(action.device):
        check(_lib.lib().ic3_random_actions(ptr(action), int(naction), int(seed) & 0xffffffff, int(env_id_offset),
                                            int(episode), int(t), E, N, stream()))
    return action
