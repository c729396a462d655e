"""The update half without autograd — /root/reference/trainer.py:128-225 (`compute_grad`) for the recurrent CommNet /
IC3Net policy (/root/reference/comm.py:134-244), as an explicit backward-through-time over what a NO-GRAD rollout
recorded.

The reference (and round 1/2 here) keeps the autograd graph of the whole rollout: every intermediate of every step —
encoder output, communication vectors, gate pre-activations, log-softmax inputs — stays alive until `loss.backward()`
(59.5 GB for one PP-hard update at 8192 envs), and the rollout has to run through differentiable ops, i.e. not through
the one-launch kernel.  Here the rollout is the ordinary rollout (ic3_policy_step where it applies) and records per step
only what cannot be re-derived: the recurrent state (h, c) that ENTERED the step, a snapshot of the env's integer state
(a few hundred bytes per env) and the two masks.  The backward pass walks the steps in reverse and, per step,
  re-evaluates   enc (ic3_env_encode_at on the snapshot), comm (ic3_comm_masked_mean), inp, the gate pre-activations
  backpropagates heads -> LSTM cell (ic3_lstm_cell_backward: dgates, dc) -> [W_ih | W_hh] -> C -> comm (its mixing matrix
                 is symmetric: the same kernel on the gradient) -> encoder (ic3_env_encode_backward on the snapshot)
with the hidden state cut every `detach_gap` steps exactly where the reference detaches it (trainer.py:56-60).  The dense
products are plain library GEMMs (hipBLASLt fp32 MFMA through torch.mm / addmm_: [R x 4H] x [4H x 2H] and its
transposes — there is nothing to fuse into them that the HBM traffic of their operands would notice); everything
pointwise or sparse is a HIP kernel of libic3rollout.

comm_passes > 1 (round 18): a lock-step window of such a policy runs no library product — _backward_window_multipass re-evaluates the
inner passes of all steps window-wide (ops.policy_forward_record) and differentiates them through ops.bptt_passes_backward, in chunks
of whole steps; PP-hard with 2 passes at 8192 envs: 144-146 ms per update instead of 222-223 (profiles/r18/multipass_window.txt).
Collection-mode windows of these policies keep the per-step loop above (_backward_episode_multipass).

Cost per step (PP-hard): forward 0.30 GFLOP-equivalents of one gate GEMM, backward = recompute (1x) + input gradient (1x)
+ weight gradient (1x): fp32 arithmetic bounds the update at ~4x the rollout's matrix work.
"""
import contextlib

import torch

from . import ops


def _is_baseline(net):
    from . import models
    return isinstance(net, models.MLP)


def supported(args, net, raw):
    """Recurrent LSTM CommNet / IC3Net (any number of communication passes), or the NON-recurrent CommNet module (round 4:
    `_backward_episode_commnet`), with the sparse encoder bound to this env."""
    if _is_baseline(net):
        # IC / IRIC baselines (models.MLP / models.RNN, no communication): round 4, _backward_episode_baseline
        if args.hid_size % 4 or not hasattr(raw, 'encode_at') or getattr(net, 'continuous', False):
            return False
        if getattr(net.obs_encoder, '__self__', None) is not raw or args.nagents != raw.nagents_env:
            return False
        if getattr(args, 'recurrent', False) and getattr(args, 'rnn_type', 'MLP') == 'LSTM':
            h4 = args.hid_size // 4
            if h4 > 64 or h4 & (h4 - 1):                          # ic3_lstm_cell_backward
                return False
        return net.affine1.weight.is_cuda and net.affine1.weight.dtype == torch.float32
    if not getattr(args, 'recurrent', False):
        if not (hasattr(net, 'f_modules') and hasattr(net, '_commnet_cache')) or getattr(net, 'continuous', False):
            return False
        if not hasattr(raw, 'encode_at') or not ops.commnet_forward_supported(args.hid_size, net.nagents):
            return False
        if getattr(net.obs_encoder, '__self__', None) is not raw or net.nagents != raw.nagents_env:
            return False
        return net.encoder.weight.is_cuda and net.encoder.weight.dtype == torch.float32
    if not (getattr(args, 'recurrent', False) and getattr(args, 'rnn_type', '') == 'LSTM' and hasattr(net, 'f_module')):
        return False
    if getattr(net, 'comm_passes', 1) < 1 or args.hid_size % 4 or not hasattr(raw, 'encode_at'):
        return False
    h4 = args.hid_size // 4
    if h4 > 64 or h4 & (h4 - 1):        # ic3_lstm_cell_backward (the non-fused step): H/4 a power of two <= 64;
        return False                    # other sizes keep the autograd update
    if getattr(net.obs_encoder, '__self__', None) is not raw or net.nagents != raw.nagents_env:
        return False
    return net.encoder.weight.is_cuda and net.encoder.weight.dtype == torch.float32


class EpisodeRecord(object):
    """What one batched episode leaves behind for the backward pass: (h, c) entering every step, the env state of every
    step, the masks of the communication block."""

    def __init__(self, T, R, H, state_words, device, recurrent=True):
        self.recurrent = recurrent
        if recurrent:
            self.hs = torch.empty((T + 1, R, H), dtype=torch.float32, device=device)     # slot t: h entering step t; slot T: h_T
            self.cs = torch.empty((T + 1, R, H), dtype=torch.float32, device=device)
        else:                                  # the non-recurrent module carries no state between steps: env snapshots + masks only
            self.hs = self.cs = None
            self.rows, self.device = R, device
        self.snaps = torch.empty((T, state_words), dtype=torch.int32, device=device)
        self.alive = [None] * T
        self.gate = [None] * T
        self.h_last = None
        self.n = 0
        # (T, R, 4H) the activated gates of every step's LSTM cell and (T, R, 2H) the inp half of its [inp | h] rows (hid 256: (T, R, H),
        # the inp rows alone — ops.record_xh_width), stored by
        # the step launch itself (ic3_env_set_record_out: Trainer._record_gates) — the backward then skips the gate product and
        # what leads up to it; gates_n = the steps that stored theirs
        self.gates = None
        self.xh = None
        self.gates_n = 0
        self.stream = None     # collection mode (Trainer._run_batch_streams): per-slot cuts of the recurrence, see backward_episode
        # (T, R, OT) the [log-probs | value] rows of every step, written by the one-launch steps themselves (Trainer hands slice t
        # as their `out`); out_n = the steps that did
        self.out = None
        self.out_n = 0
        # (T, R, H) the hidden state every step of a NON-recurrent baseline (models.MLP) ended with, written by the step launch itself
        # (Trainer hands slot t as ic3_commnet_step's h_out); h_fin_n = the steps that did — _backward_window_mlp reads it
        self.h_fin = None
        self.h_fin_n = 0
        # comm_passes = P in 2..4 (Trainer._record_passes, args.window_record_passes): what every pass of every step of the window
        # launch computed, stored by that launch itself (ops.policy_step_window's record_passes) — pass_gates (P, T, R, 4H) the
        # activated gates, pass_inp (P, T, R, 2H) the inp half of the [inp | h] rows, pass_h / pass_c (P - 1, T, R, H) the state
        # ENTERING pass i at entry i - 1 (pass 0 enters on slot t of hs / cs); pass_n = the steps that wrote theirs.  The window
        # backward reads them instead of re-evaluating the passes where pass_n == n, and the gates are its dgates afterwards (it
        # then sets pass_n back to 0: a second backward over the record re-evaluates)
        self.pass_gates = self.pass_inp = self.pass_h = self.pass_c = None
        self.pass_n = 0

    def release(self):
        """Drop the record's tensors now (tens of GB with recorded gates): the update is done with them, and whatever still
        refers to the record object — a reference cycle waiting for the garbage collector — must not keep them alive beside
        the next update's record."""
        self.hs = self.cs = self.gates = self.xh = self.snaps = self.h_last = self.out = self.h_fin = None
        self.pass_gates = self.pass_inp = self.pass_h = self.pass_c = None
        self.pass_n = 0
        self.alive, self.gate, self.stream = [], [], None

    def start_from(self, h, c):
        """Collection mode: this window continues the streams of the previous one — the state it ended with is the state
        entering slot 0 (an env that starts an episode there is zeroed inside the step launch, and again in the backward)."""
        R, H = self.hs.shape[1:]
        if h.shape[-1] != H:
            self._put(self.hs[0], h)
            self._put(self.cs[0], c)
        else:
            self.hs[0].copy_(h.detach().reshape(R, H))
            self.cs[0].copy_(c.detach().reshape(R, H))
        return (self.hs[0], self.cs[0])

    def start(self):
        """Zero state of step 0, held in the record itself: a rollout that reads (h, c) from slot t and lets the step launch
        write slot t + 1 (ic3_env_set_hidden_out) records the recurrent state without a single copy."""
        self.hs[0].zero_()
        self.cs[0].zero_()
        return (self.hs[0], self.cs[0])

    def slot(self, t):
        return (self.hs[t], self.cs[t])

    def h_out(self, t):
        """h LEAVING step t: the state entering step t + 1, or what the rollout ended with"""
        return self.hs[t + 1] if t + 1 < self.n else self.h_last

    def h_last_is_slot(self, T):
        """h_last IS slot T of the record (the in-place rollout wrote it there): h leaving the steps is hs[1:T + 1] then"""
        return self.h_last is not None and self.hs.shape[0] > T and self.h_last.data_ptr() == self.hs[T].data_ptr()

    def record(self, t, net, raw, prev_hid, info):
        if self.recurrent:
            h, c = prev_hid if isinstance(prev_hid, (tuple, list)) else (prev_hid, None)   # (models.RNN, rnn_type MLP: h only)
            R, H = self.hs.shape[1:]
            if h.shape[-1] != H:                               # a zero-padded twin's record, an (R, hid_size) state
                self._put(self.hs[t], h)
                if c is not None:
                    self._put(self.cs[t], c)
            elif h.data_ptr() != self.hs[t].data_ptr():        # (in-place rollouts hand slot t itself)
                self.hs[t].copy_(h.detach().reshape(R, H))
                if c is not None:
                    self.cs[t].copy_(c.detach().reshape(R, H))
            dev = self.hs.device
        else:
            R, dev = self.rows, self.device
        raw.snapshot(out=self.snaps[t])
        if hasattr(net, '_mask'):                              # the communication block's masks (CommNetMLP)
            E = R // net.nagents
            self.alive[t] = net._mask(info, 'alive_mask', E, dev)
            self.gate[t] = net._mask(info, 'comm_action', E, dev) if net.args.hard_attn else None
        self.n = t + 1

    @staticmethod
    def _put(slot, x):
        """slot (R, wide) <- x (R, narrower), zero beyond"""
        slot.zero_()
        slot[:, :x.shape[-1]].copy_(x.detach().reshape(slot.shape[0], x.shape[-1]))

    def finish(self, prev_hid):
        if not self.recurrent:
            return
        h = prev_hid[0] if isinstance(prev_hid, (tuple, list)) else prev_hid
        if h.shape[-1] != self.hs.shape[2]:
            self.h_last = torch.empty_like(self.hs[0])
            self._put(self.h_last, h)
        elif self.n < self.hs.shape[0] and h.data_ptr() == self.hs[self.n].data_ptr():
            self.h_last = self.hs[self.n]
        else:
            self.h_last = h.detach().reshape(self.hs.shape[1:]).clone()


def _returns(args, rewards, episode_masks, episode_mini_masks):
    """trainer.py:162-171: the reversed scan of the cooperative and the per-agent returns and their mix — one launch
    (ic3_returns_scan) on the GPU for up to 256 agents, the reference's loop otherwise."""
    T, E, n = rewards.shape
    if rewards.is_cuda and n <= 256 and rewards.dtype == torch.float32:
        return ops.returns_scan(rewards, episode_masks, episode_mini_masks, args.gamma, args.mean_ratio)
    coop_returns = torch.empty_like(rewards)
    ncoop_returns = torch.empty_like(rewards)
    prev_coop = torch.zeros_like(rewards[0])
    prev_ncoop = torch.zeros_like(rewards[0])
    for i in reversed(range(T)):
        coop_returns[i] = rewards[i] + args.gamma * prev_coop * episode_masks[i]
        ncoop_returns[i] = rewards[i] + args.gamma * prev_ncoop * episode_masks[i] * episode_mini_masks[i]
        prev_coop = coop_returns[i]
        prev_ncoop = ncoop_returns[i]
    return args.mean_ratio * coop_returns.mean(dim=2, keepdim=True) + (1 - args.mean_ratio) * ncoop_returns


def _recorded_out(records, T):
    """The (T, R, OT) rows the step launches of the batch's episodes wrote, when every step wrote into its record's buffer
    (Trainer: EpisodeRecord.out) — no stack of T x heads views then."""
    if not records or any(getattr(r, 'out', None) is None or r.out_n != r.n for r in records) or sum(r.n for r in records) != T:
        return None
    return records[0].out[:records[0].n] if len(records) == 1 else torch.cat([r.out[:r.n] for r in records])


def loss_gradients(args, batch, records=None):
    """trainer.py:128-218 up to the losses: returns (stat, d_out) with d_out (T, R, OT) = dL/d[logits of every head |
    value] of every transition (the log-softmax is folded in: gradients w.r.t. its INPUT).  On the device, with the step
    launches' rows at hand (`records`) and at most four heads: ONE launch (ic3_loss_gradients) behind the return scan; the tensor
    program below is the same arithmetic (tests/test_trainer_gpu.py compares them)."""
    n = args.nagents
    rewards = torch.stack(batch.reward)                                   # (T, E, N)
    T, E = rewards.shape[0], rewards.shape[1]
    episode_masks = torch.stack(batch.episode_mask)
    episode_mini_masks = torch.stack(batch.episode_mini_mask)
    out_rows = _recorded_out(records, T) if (rewards.is_cuda and bool(getattr(args, 'fused_loss', True))) else None
    # (ic3_loss_gradients keeps a transition's [logits | value] row in 16 registers: wider rows take the tensor program)
    if out_rows is not None and len(batch.action_out[0]) <= 4 and out_rows.shape[-1] <= 16 and rewards.dtype == torch.float32:
        actions = torch.stack(batch.action).reshape(T, -1, E * n)             # (T, heads, R) int32
        alive_masks = torch.stack([m['alive_mask'] for m in batch.misc]).reshape(T, E * n)
        live = torch.stack([m['live'] for m in batch.misc])                   # (T, E)
        returns = _returns(args, rewards, episode_masks, episode_mini_masks).reshape(T, E * n)
        shift, scale = 0.0, 1.0
        if args.normalize_rewards:                                        # trainer.py:176-177 (live entries only)
            lv = live.unsqueeze(2).expand(T, E, n).reshape(T, E * n)
            adv = returns - out_rows[:, :, -1]
            cnt = lv.sum()
            mean = (adv * lv).sum() / cnt
            var = (((adv - mean) ** 2) * lv).sum() / (cnt - 1)
            shift, scale = float(mean), float(1.0 / var.sqrt())
        if actions.dtype != torch.int32:
            actions = actions.int()
        d_out, sums = ops.loss_gradients(out_rows, actions.contiguous(), returns.contiguous(), alive_masks.contiguous(),
                                         live.contiguous(), [int(a) for a in args.naction_heads], float(args.entr),
                                         float(args.value_coeff), shift, scale)
        sums = sums.tolist()
        return dict(action_loss=sums[0], value_loss=sums[1], entropy=sums[2]), d_out
    actions = torch.stack(batch.action).permute(0, 2, 3, 1).long()        # (T, E, N, heads)
    values = torch.stack([v.reshape(E, n) for v in batch.value])          # (T, E, N)
    nheads = len(batch.action_out[0])
    log_p_a = [torch.stack([ao[k] for ao in batch.action_out]) for k in range(nheads)]    # (T, E, N, A_k)
    alive_masks = torch.stack([m['alive_mask'] for m in batch.misc])      # (T, E, N), already x live
    live = torch.stack([m['live'] for m in batch.misc]).unsqueeze(2).expand(T, E, n)

    returns = _returns(args, rewards, episode_masks, episode_mini_masks)  # trainer.py:162-171
    advantages = returns - values                                         # trainer.py:173-174 (values carry no graph here)
    if args.normalize_rewards:                                            # trainer.py:176-177 (live entries only)
        cnt = live.sum()
        mean = (advantages * live).sum() / cnt
        var = (((advantages - mean) ** 2) * live).sum() / (cnt - 1)
        advantages = (advantages - mean) / var.sqrt()
    stat = dict()
    per_head = [lp.gather(3, actions[..., k:k + 1]).squeeze(3) for k, lp in enumerate(log_p_a)]
    if args.advantages_per_action:                                        # trainer.py:192-197 (the same sum either way)
        action_loss = sum((-advantages * lp * alive_masks).sum() for lp in per_head)
    else:
        action_loss = (-advantages * sum(per_head) * alive_masks).sum()
    value_loss = ((values - returns).pow(2) * alive_masks).sum()          # trainer.py:203-206
    entropy = 0
    for lp in log_p_a:                                                    # trainer.py:211-218 (no alive mask there)
        entropy = entropy - (lp * lp.exp() * live.unsqueeze(3)).sum()
    stat['action_loss'] = action_loss.item()
    stat['value_loss'] = value_loss.item()
    stat['entropy'] = entropy.item()

    cols = []
    w_act = (-advantages * alive_masks).unsqueeze(3)                      # d action_loss / d logp[a]
    for k, lp in enumerate(log_p_a):
        dlp = torch.zeros_like(lp)
        dlp.scatter_(3, actions[..., k:k + 1], w_act)
        if args.entr > 0:                                                 # loss -= entr * entropy
            dlp = dlp + args.entr * live.unsqueeze(3) * lp.exp() * (lp + 1.0)
        cols.append(dlp - lp.exp() * dlp.sum(3, keepdim=True))            # through log_softmax: gradient w.r.t. the logits
    cols.append((2.0 * args.value_coeff * (values - returns) * alive_masks).unsqueeze(3))
    d_out = torch.cat(cols, 3).reshape(T, E * n, -1).contiguous()
    return stat, d_out


def backward_episode(args, net, raw, rec, d_out, acc, carry=None):
    """Backward through one recorded episode; parameter gradients are ADDED into `acc` (fp32 tensors keyed like the
    fused weight cache).

    The recurrence is cut where `_Cuts` says — detach points, and in collection mode (`rec.stream`, every policy family: the
    non-recurrent ones have no state to cut, only the masks of a starting env) the starting envs and episode ends inside the
    window; there `carry` = (dL/dh, dL/dc) arriving at the window's last slot from the next window, and the pair leaving the
    window's first slot is returned."""
    if _is_baseline(net):
        si = standin_for_backward(args, net, rec)
        if si is not None:
            return _backward_episode_standin(net, si, raw, rec, d_out, acc, carry)
        if _rnn_window_ok(args, net, raw, rec, d_out):
            return _backward_window_rnn(args, net, raw, rec, d_out, acc, carry)
        return _backward_episode_baseline(args, net, raw, rec, d_out, acc, carry)
    if not rec.recurrent:
        return _backward_episode_commnet(args, net, raw, rec, d_out, acc)
    if net.comm_passes > 1:
        if _multipass_window_ok(args, net, raw, rec, d_out):
            return _backward_window_multipass(args, net, raw, rec, d_out, acc, carry)
        net.multipass_loop_backwards = getattr(net, 'multipass_loop_backwards', 0) + 1
        return _backward_episode_multipass(args, net, raw, rec, d_out, acc, carry)
    fc = net._fused_cache()
    T, R, H = rec.n, rec.hs.shape[1], rec.hs.shape[2]
    N = net.nagents
    E = R // N
    dev = rec.hs.device
    mode_avg = getattr(args, 'comm_mode', 'avg') == 'avg'
    mask_zero = bool(args.comm_mask_zero)
    w_cat_t = fc['w_cat_t']                                               # (2H, 4H) = [W_ih | W_hh]^T
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    xh, comm, dgates = z(R, 2 * H), z(E, N, H), z(R, 4 * H)   # xh = [inp | h_{t-1}]
    dxh, dcomm = z(R, 2 * H), z(R, H)                                      # dxh = [d inp | d h_{t-1}]
    inp, dinp = xh[:, :H], dxh[:, :H]
    # gate recompute + cell backward in one launch when the packed gate weights of the rollout kernel exist (hid 64/128/256);
    # its bias partials accumulate over the episode's steps and are reduced once, behind the loop
    fused_gates = fc.get('ps_l_wp') is not None and ops.lstm_gates_backward_supported(H) and R * 4 * H * 4 < 2 ** 32
    # the input gradient of the gate product inside the same launch (ic3_lstm_gates_backward_dx: split mode, hid 64 / 128)
    fused_dx = fused_gates and fc.get('ps_l_wp3') is not None and fc.get('ps_l_wp3_bwd') is not None and \
        bool(getattr(args, 'fused_input_grad', True))
    # the gates of every step as the rollout recorded them: no gate product in the backward at all
    given = fused_dx and rec.gates is not None and rec.xh is not None and rec.gates_n == T and rec.gates.shape[2] == 4 * H
    # ... and then the whole window as ONE host call (round 6: ic3_bptt_backward — three launches per step, no library product,
    # nothing on the host between them; the weight gradient of the window in one launch behind it)
    if given and bool(getattr(args, 'bptt_native_loop', True)) and d_out.shape[-1] <= 16 and ops.bptt_backward_supported(raw, H):
        return _backward_window_native(args, net, raw, rec, d_out, acc, carry, fc)
    if H == 256:
        # (ic3_lstm_gates_backward_dx takes hid 64 / 128: at 256 the input gradient's split planes serve the window path alone,
        #  and its record holds inp rows only (ops.record_xh_width), not the per-step loop's [inp | h] — the recomputing loop)
        fused_dx = given = False
    if fused_gates:
        bias_parts = torch.zeros(((R + 63) // 64, 4 * H), dtype=torch.float32, device=dev)
    else:
        gates, bias_parts, bsum = z(R, 4 * H), z(ops.LSTM_BWD_MAX_PARTIALS, 4 * H), z(4 * H)
    wgrad = _RowBlockGrad(acc['w_cat_t'], R, 8)                           # xh^T . dgates
    cgrad = None if mask_zero else _RowBlockGrad(acc['c_w'], R, 32)       # d inp^T . comm
    dh_rec = torch.zeros((R, H), dtype=torch.float32, device=dev)         # dL/dh_t, dL/dc_t arriving from step t + 1
    dc_rec = torch.zeros((R, H), dtype=torch.float32, device=dev)
    enc_grad = _EncoderGrad(raw, acc, 'wt', 'enc_bias')
    cuts = _Cuts(args, rec, T, E, N, dev)
    # collection mode on recorded gates: the per-row cuts ride inside the launches that touch the rows anyway
    # (ic3_lstm_gates_backward_given: row_live, row_keep; ic3_comm_masked_mean_add: out_row_scale) — no passes of their own;
    # the state that entered a starting env stays in the record (the launch multiplies it by row_live)
    cut_in_kernel = cuts.on and given
    cuts.carry_in(carry, dh_rec, dc_rec, at_border=cut_in_kernel)
    if cuts.on:
        _heads_grad_episode(rec, d_out, acc, T, R, H)                     # (reads h_t of every slot: before rows are zeroed)
    for t in reversed(range(T)):
        h_prev, c_prev = rec.hs[t], rec.cs[t]
        if not cut_in_kernel:
            cuts.cut(t, dh_rec, dc_rec)
            cuts.entering(t, h_prev, c_prev)
        alive, gate = cuts.masks(t, rec.alive[t], rec.gate[t], fill_gate=cut_in_kernel)
        # ---- the forward of step t again: enc + C.bias -> inp, comm, gate pre-activations (comm.py:119,181-215)
        if given:                                                         # inp as the step launch stored it; comm for C's gradient
            xh = rec.xh[t]
            if not mask_zero:
                ops.comm_masked_mean_raw(h_prev.view(E, N, H), alive, gate, mode_avg, True, out=comm)
        else:
            raw.encode_at(rec.snaps[t], fc['wt'], fc['enc_bias'], out=inp, loc_table=fc['loc_table'])
            if not fused_gates:
                xh[:, H:].copy_(h_prev)                                   # (the fused gate launch fills it)
            if mask_zero:
                comm.zero_()                                              # comm.py:40-41: C sees zeros
            else:
                ops.comm_masked_mean_raw(h_prev.view(E, N, H), alive, gate, mode_avg, True, out=comm)
                inp.addmm_(comm.view(R, H), fc['c_wt'])
        if not fused_gates:
            torch.addmm(fc['b_cat'], xh, w_cat_t, out=gates)              # one K = 2H product, as in the rollout
        # ---- heads (comm.py:228,239) -> LSTM cell
        d = d_out[t]
        # dL/dh_t = what step t + 1 sent back + the heads' share — in place (addmm with another `out` first copies R x H floats);
        # dh_rec is rewritten with dL/dh_{t-1} at the end of the iteration, after the cell backward has consumed it
        dh = dh_rec.addmm_(d, fc['w_heads'])
        if given:                                                         # dc_rec <- dL/dc_{t-1}
            ops.lstm_gates_backward_given(rec.gates[t], c_prev, dh, dc_rec, dgates, dc_rec, bias_parts, True, xh=xh, h_prev=h_prev,
                                          lstm_wp3_bwd=fc['ps_l_wp3_bwd'], dxh=dxh,
                                          row_live=cuts.live_flat[t] if cut_in_kernel else None,
                                          row_keep=cuts.keep_flat[t] if cut_in_kernel else None)
        elif fused_gates:
            # (the heads' own weight gradient is one pass over the whole episode behind the loop: ic3_heads_grad)
            ops.lstm_gates_backward(xh, fc['ps_l_wp'], fc['b_cat'], c_prev, dh, dc_rec, dgates, dc_rec, bias_parts, True,
                                    h_prev=h_prev, lstm_wp3=fc.get('ps_l_wp3'), lstm_wp3_bwd=fc.get('ps_l_wp3_bwd') if fused_dx else None,
                                    dxh=dxh if fused_dx else None)
        else:
            if not cuts.on:
                acc['w_heads'].addmm_(d.t(), rec.h_out(t))
                acc['b_heads'].add_(d.sum(0))
            parts = ops.lstm_cell_backward(gates, c_prev, dh, dc_rec, dgates, dc_rec, bias_parts)
            torch.sum(parts, 0, out=bsum)
            acc['b_cat'].add_(bsum)
        # ---- [W_ih | W_hh] (torch.nn.LSTMCell): weight gradient and input gradient, one product each
        wgrad.add(xh, dgates)                                             # (2H, R) x (R, 4H)
        if not fused_dx:
            torch.mm(dgates, w_cat_t.t(), out=dxh)                        # (R, 4H) x (4H, 2H) -> [d inp | d h_{t-1}]
        # ---- inp = encoder(obs) + C(comm) (+ both biases)
        if not mask_zero:
            cgrad.add(dinp, comm.view(R, H))
            torch.mm(dinp, fc['c_wt'].t(), out=dcomm)                     # d comm = d inp . C.weight
            # dL/dh_{t-1} (what step t - 1 receives) = d h of the gate product + the communication block's share, one pass
            ops.comm_masked_mean_raw(dcomm.view(E, N, H), alive, gate, mode_avg, True, out=dh_rec.view(E, N, H), addend=dxh[:, H:],
                                     row_scale=cuts.keep_flat[t - 1] if cut_in_kernel and t > 0 else None)
        elif cut_in_kernel and t > 0:
            torch.mul(dxh[:, H:], cuts.keep_rows[t - 1], out=dh_rec)
        else:
            dh_rec.copy_(dxh[:, H:])
        enc_grad.step(dinp, rec.snaps[t])
    enc_grad.finish(H)
    wgrad.finish()
    if cgrad is not None:
        cgrad.finish()
    if fused_gates:
        acc['b_cat'].add_(bias_parts.sum(0))
        if not cuts.on:
            _heads_grad_episode(rec, d_out, acc, T, R, H)
    return (dh_rec, dc_rec)       # dL/d(h, c) entering the record's first slot (collection mode: the previous window's carry)


def _dhead_rows(d_out, T):
    """d_out's first T steps as one contiguous block: a view where they are one already."""
    d = d_out[:T]
    return d if d.is_contiguous() else d.contiguous()


def _enc_window(args, raw, H):
    """The sparse encoder's backward runs in its window form: asked for (args.enc_window, on by default) and there for this env."""
    return bool(getattr(args, 'enc_window', True)) and raw.encode_window_work(H) is not None


def _backward_window_native(args, net, raw, rec, d_out, acc, carry, fc):
    """backward_episode on recorded gates through ic3_bptt_backward (csrc/bptt_kernels.hip).  Per step, last to first:
      ic3_lstm_gates_backward_given   cell derivative from the recorded gates, IN PLACE (dgates over the gates), dL/dh_t taking the
                                      heads' share d_t . W_heads on the way in, [d inp | d h_direct] = dgates . [W_ih | W_hh]
      ic3_comm_backward               dL/dh_{t-1} = d h_direct + (M d inp) . C,  dC += (M d inp)^T h_{t-1}   (M: the mixing matrix of
                                      the communication block, symmetric — one mix feeds both products; comm itself is never formed)
      ic3_env_encode_backward_accumulate   the sparse encoder's stage 1 on the step's snapshot — or, with the steps' input gradients
                                      kept in a ring, ONE ic3_env_encode_backward_window launch over all of them behind the loop
    and behind the loop ONE weight-gradient launch over the window's T x R rows (the record's inp rows, the recorded h, the
    dgates now standing in the gate record), the heads' pass, the encoder's expansion, the partials' sums.  Same cuts as
    backward_episode (detach points; collection mode: row_live / row_keep / gated-off fresh envs)."""
    T, R, H = rec.n, rec.hs.shape[1], rec.hs.shape[2]
    N = net.nagents
    E = R // N
    dev = rec.hs.device
    mode_avg = getattr(args, 'comm_mode', 'avg') == 'avg'
    mask_zero = bool(args.comm_mask_zero)
    zeros = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
    dh_rec, dc_rec = zeros(R, H), zeros(R, H)
    # the per-step input gradients: a ring of T of them when the encoder's backward has its window form (one launch over all the
    # window's states behind the loop instead of one per step) and the memory is there, else one buffer
    ring = _enc_window(args, raw, H) and _ring_fits(dev, T * R * 2 * H * 4)
    dxh = torch.empty((T, R, 2 * H) if ring else (R, 2 * H), dtype=torch.float32, device=dev)
    bias_parts = zeros((R + 63) // 64, 4 * H)
    # two chains of launches (envs [0, E1) and [E1, E) on two streams): one fills the ragged last round of the other's launches
    two = ring and bool(getattr(args, 'bptt_two_chains', True)) and ops.first_chain_envs(E, N) < E
    # args.backward_walk_lstm: a window without communication (IRIC's LSTM cell on its stand-in, --comm_mask_zero) with the ring — its
    # 2 T launches (gate launch + the copy of d h_prev, per step and chain) as ONE (an ic3_bptt_walk descriptor: every 64-row tile
    # walked last step to first by one workgroup, dL/dh on chip), one stream, the same gradients bit for bit.  Not under bench's
    # per-gate events (raw.gate_timer): they have no meaning in one launch
    gate_timer = getattr(raw, 'gate_timer', None)
    walk = bool(getattr(args, 'backward_walk_lstm', 0)) and mask_zero and ring and gate_timer is None
    if walk:
        two = False
    dcw_parts = None if mask_zero else zeros(ops.bptt_dcw_partials(E, N, two), H, H)
    cuts = _Cuts(args, rec, T, E, N, dev)
    cuts.carry_in(carry, dh_rec, dc_rec, at_border=True)
    alive, gate = cuts.masks_window(rec.alive[:T], rec.gate[:T])
    dhead = d_out if d_out.is_contiguous() else d_out.contiguous()
    with _heads_grad_beside(args, rec, d_out, acc, T, R, H):
        ops.bptt_backward(raw, T, E, N, H, rec.gates, rec.hs, rec.cs, dhead, rec.snaps, alive, gate, fc['ps_l_wp3_bwd'], fc['w_heads'],
                          None if mask_zero else net.C_modules[0].weight.detach(), dh_rec, dc_rec, dxh, bias_parts, dcw_parts,
                          mode_avg=mode_avg, comm_zero=mask_zero, detach_gap=cuts.gap, row_live=cuts.live_flat,
                          row_keep=cuts.keep_flat, enc_first=True,
                          gate_events=gate_timer,     # (bench.py --mode train: HIP events around the gate launches)
                          two_chains=two, walk=walk)
        if H == 256 and not bool(getattr(args, 'lstm_wgrad_kernel', True)):
            _weight_grad_products(rec, T, R, H, acc['w_cat_t'], cuts.live_flat)
        else:
            work = acc.setdefault('_work', {})
            ops.lstm_weight_grad(rec.xh[:T], rec.hs[:T], rec.gates[:T], acc['w_cat_t'], row_live=cuts.live_flat, accumulate=True,
                                 work=work, split=bool(getattr(args, 'gate_split', True)))
        dwt, db = raw.encode_backward_window_finish(H, want_bias=True) if ring else raw.encode_backward_finish(H, want_bias=True)
        acc['wt'].add_(dwt)
        acc['enc_bias'].add_(db)
        acc['b_cat'].add_(bias_parts.sum(0))
        if not mask_zero:
            acc['c_w'].add_(dcw_parts.sum(0))
    if walk:
        net.lstm_backward_walks = getattr(net, 'lstm_backward_walks', 0) + 1
    return (dh_rec, dc_rec)


def _weight_grad_products(rec, T, R, H, dW, row_live):
    """The window's [W_ih | W_hh] gradient at hid 256 behind args.lstm_wgrad_kernel=False (the default is the kernel,
    ops.lstm_weight_grad, as at 64 / 128): two library products over all T x R rows at once, behind the loop — dW[:H] += inp^T . dgates, dW[H:] += (row_live h)^T . dgates.  Collection mode scales the
    dgates rows by row_live in place once the inp product has read them (the record is not read again): no T x R x H copy of h."""
    Q = T * R
    dg = rec.gates[:T].view(Q, 4 * H)
    dW[:H].addmm_(rec.xh[:T].reshape(Q, H).t(), dg)
    if row_live is not None:
        dg.mul_(row_live.view(Q, 1))
    dW[H:].addmm_(rec.hs[:T].reshape(Q, H).t(), dg)


_SIDE_STREAMS = {}     # per device: the stream the heads' gradient runs on beside the backward's chain


@contextlib.contextmanager
def _heads_grad_beside(args, rec, d_out, acc, T, R, H):
    """The heads' weight gradient of a window backward.  It reads only d_out and the recorded h, so it runs on a second stream
    BESIDE the chain issued in the `with` body (no LDS, a few waves per CU: it fits next to the chain's workgroups and rides their
    idle issue slots instead of taking 0.7 ms of its own).  The current stream waits for it on the way out WHETHER OR NOT the body
    raised: the caller releases the record then, and the side stream must be done reading hs / d_out and writing acc['w_heads'].
    Without a second stream (CPU, args.heads_grad_beside off, a graph capture) the pass runs behind the body, if that succeeded."""
    dev = rec.hs.device if rec.hs is not None else rec.h_fin.device
    side = None
    try:
        if dev.type == 'cuda' and bool(getattr(args, 'heads_grad_beside', True)) and not torch.cuda.is_current_stream_capturing():
            side = _SIDE_STREAMS.get(dev.index)
            if side is None:
                side = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                _heads_grad_episode(rec, d_out, acc, T, R, H)
        yield
    finally:
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)
    if side is None:
        _heads_grad_episode(rec, d_out, acc, T, R, H)


def device_room(dev):
    """Bytes the device can still give: what it has free + the blocks the caching allocator holds unused."""
    free, _ = torch.cuda.mem_get_info(dev)
    return free + max(torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev), 0)


def _ring_fits(dev, nbytes):
    """Room for the ring of per-step input gradients: a quarter of what the device can still give."""
    return dev.type != 'cuda' or nbytes <= device_room(dev) // 4


class _Cuts(object):
    """Where the recurrence of a record of T steps is cut, for every backward driver.
    Lock-step: the gradient of the state leaving step t is dropped where the Trainer hands the state on detached, (t + 1) %
    detach_gap == 0 (trainer.py:56-60).
    Collection mode (rec.stream, Trainer._run_batch_streams: the record is a WINDOW of consecutive slots of E streams of
    episodes): an env that STARTS an episode at slot t has nobody dead, its agents gated off and a zero state entering
    (trainer.py:38-51, quirks Q21 / Q22), as the step launch had it; `keep[t]` marks the envs whose state leaving slot t reaches
    slot t + 1 with its gradient (no episode end, no detach point of the env's OWN step counter).
    `live_flat` / `keep_flat`: the (T, R) row factors the kernels take (None in lock-step); `gap`: the detach_gap left for the
    host calls and `cut` to apply — 0 where the cuts ride in `keep` or none falls inside the record."""

    def __init__(self, args, rec, T, E, N, dev):
        st = rec.stream
        self.on = st is not None
        gap = int(getattr(args, 'detach_gap', 10000))
        self.gap = 0 if self.on or gap > T else gap
        self.live_flat = self.keep_flat = None
        if not self.on:
            return
        self.T, self.shape, self.dev, self._consts = T, (E, N), dev, None
        self.fresh = st['fresh'][:T]                                                     # (T, E) bool
        self.live_flat = (~self.fresh).to(torch.float32).repeat_interleave(N, dim=1).contiguous()
        self.keep_flat = st['keep'][:T].to(torch.float32).repeat_interleave(N, dim=1).contiguous()
        self.live_rows, self.keep_rows = self.live_flat.unsqueeze(2), self.keep_flat.unsqueeze(2)   # (T, R, 1)

    def _ones_zeros(self):
        if self._consts is None:
            ones = torch.ones(self.shape, dtype=torch.int32, device=self.dev)
            self._consts = (ones, torch.zeros_like(ones))
        return self._consts

    def carry_in(self, carry, dh, dc=None, at_border=False):
        """Collection mode: (dL/dh, dL/dc) arriving at the window's last slot from the next window; `at_border`: cut where it
        crosses into the window (the drivers whose kernels apply keep[t - 1] on the way OUT of slot t — the loops cut per step)."""
        if not self.on:
            return
        if carry is not None:
            dh.copy_(carry[0])
            if dc is not None:
                dc.copy_(carry[1])
        if at_border:
            dh.mul_(self.keep_rows[self.T - 1])

    def masks(self, t, alive, gate, fill_gate=False):
        """The step's masks with the starting envs' rows set: nobody is dead (Q21), the agents are gated off — what the zero state
        entering the slot amounts to for the communication block (Q22).  `fill_gate`: a missing gate counts as all ones first
        (the entering state stays in the record there, so gating off is what hides it)."""
        if not self.on:
            return alive, gate
        ones, zeros = self._ones_zeros()
        fr = self.fresh[t].unsqueeze(1)
        if gate is None and fill_gate:
            gate = ones
        return (torch.where(fr, ones, alive) if alive is not None else None,
                torch.where(fr, zeros, gate) if gate is not None else None)

    def masks_window(self, alive, gate, fill_gate=True):
        """`masks` for all T steps at once — one `where` per mask over (T, E, N); returns the two lists of T.  fill_gate (the
        drivers that leave the entering state in the record): a missing gate counts as all ones first; without it a window that
        has no gate at all keeps none, as `masks` does step by step"""
        alive, gate = list(alive), list(gate)
        if not self.on:
            return alive, gate
        ones, zeros = self._ones_zeros()
        fr = self.fresh.unsqueeze(2)
        if any(m is not None for m in alive):
            alive = list(torch.where(fr, ones, torch.stack([m if m is not None else ones for m in alive])).unbind(0))
        if fill_gate or any(m is not None for m in gate):
            gate = list(torch.where(fr, zeros, torch.stack([m if m is not None else ones for m in gate])).unbind(0))
        return alive, gate

    def entering(self, t, h, c=None):
        """(h, c) entering slot t with the rows of starting envs zeroed (in place: the record is not read again)"""
        if self.on:
            h.mul_(self.live_rows[t])
            if c is not None:
                c.mul_(self.live_rows[t])
        return h, c

    def cut(self, t, *grads):
        """the gradient of the state LEAVING slot t: lock-step — zero at the episode's detach points; collection — times keep"""
        if self.on:
            for g in grads:
                g.mul_(self.keep_rows[t])
        elif self.gap and (t + 1) % self.gap == 0:
            for g in grads:
                g.zero_()

    def h_out(self, rec):
        """h leaving every step of the record, for the heads' gradient inside a loop — copies in collection mode, taken before
        `entering` zeroes rows of the record"""
        return [rec.h_out(t).clone() if self.on else rec.h_out(t) for t in range(rec.n)]


class _EncoderGrad(object):
    """The sparse encoder's weight gradient over the steps of a loop, added to acc[wkey] / acc[bkey]: the first stage per step
    into partial sums and the expansion into (obs_dim, H) once behind the loop (encode_backward_accumulate / _finish), or
    — where the env has no such form or declines — the whole gradient per step."""

    def __init__(self, raw, acc, wkey, bkey):
        self.raw, self.acc, self.keys = raw, acc, (wkey, bkey)
        self.partial = None       # None: nothing accumulated yet; True: partial sums hold the steps so far; False: per-step form

    def _add(self, dwt, db):      # (db = the sum of the rows of d: every bias that adds to the encoder's output sees it)
        self.acc[self.keys[0]].add_(dwt)
        self.acc[self.keys[1]].add_(db)

    def step(self, d, snap):
        if self.partial is not False:
            self.partial = self.raw.encode_backward_accumulate(d, snap, first=(self.partial is None)) \
                if hasattr(self.raw, 'encode_backward_accumulate') else False
        if self.partial is False:
            self._add(*self.raw.encode_backward(d, snap, want_bias=True))

    def finish(self, H):
        if self.partial:
            self._add(*self.raw.encode_backward_finish(H, want_bias=True))


class _RowBlockGrad(object):
    """dst += a^T . b summed over the steps of a loop, a (R, m) and b (R, n) — a weight gradient with K = R.  As `nb` batched
    products over row blocks, summed once behind the loop, the library fills the chip (a single (H, H) result is 24 workgroups of
    split-K; the (2H, 4H) one: 118 instead of 83 TFLOP/s at R = 81920, tools/exp/microbench_bptt_gemms.py); the plain product
    where R is small or does not divide."""

    def __init__(self, dst, R, nb):
        self.dst, self.R = dst, R
        self.nb = nb if R % nb == 0 and R >= 8192 else 1
        self.part = torch.zeros((self.nb,) + tuple(dst.shape), dtype=torch.float32, device=dst.device) if self.nb > 1 else None

    def add(self, a, b):
        if self.part is None:
            self.dst.addmm_(a.t(), b)
        else:
            rows = self.R // self.nb
            self.part.baddbmm_(a.view(self.nb, rows, a.shape[1]).transpose(1, 2), b.view(self.nb, rows, b.shape[1]))

    def finish(self):
        if self.part is not None:
            self.dst.add_(self.part.sum(0))


def _baseline_w_heads(net):
    """(OT, H): the action heads' weights over the value head's, the column order of d_out"""
    return torch.cat([hd.weight for hd in net.heads] + [net.value_head.weight], 0).detach().contiguous()


def _heads_grad_episode(rec, d_out, acc, T, R, H):
    """heads + value head over a whole record: dW += sum_t d_t^T h_t, db += sum_t sum_rows d_t — h_t of step t is the state
    ENTERING step t + 1 (slot t + 1 of the record), or slot t of h_fin where the record keeps no recurrent state (models.MLP).
    ONE pass (ic3_heads_grad) for up to 16 output columns, a library product otherwise."""
    def grad(d, h):
        if d.shape[-1] <= ops.HEADS_GRAD_MAX_OT:
            ops.heads_grad(d, h, acc['w_heads'], acc['b_heads'], acc.setdefault('_work', {}))
        else:                                                             # (more than 15 actions in total)
            acc['w_heads'].addmm_(d.t(), h)
            acc['b_heads'].add_(d.sum(0))
    if rec.hs is None:
        grad(d_out[:T].reshape(T * R, -1), rec.h_fin[:T].reshape(T * R, H))
    elif rec.h_last_is_slot(T):
        grad(d_out[:T].reshape(T * R, -1), rec.hs[1:T + 1].reshape(T * R, H))
    else:
        if T > 1:
            grad(d_out[:T - 1].reshape((T - 1) * R, -1), rec.hs[1:T].reshape((T - 1) * R, H))
        grad(d_out[T - 1], rec.h_last)


def _backward_episode_multipass(args, net, raw, rec, d_out, acc, carry=None):
    """comm_passes > 1 (comm.py:179-218): the step's passes are re-evaluated forward from the (h, c) that entered the step
    — pass i: comm_i = mix(h_i), inp_i = enc + C_i(comm_i), (h_{i+1}, c_{i+1}) = LSTMCell(inp_i, (h_i, c_i)), every pass's
    [inp | h], comm and c kept for the duration of the step — and then differentiated last pass first; the encoder sees
    the sum of the passes' d inp.  Plain launch chain (library GEMMs + the pointwise kernels): this is f3 coverage."""
    fc = net._fused_cache()
    P = net.comm_passes
    T, R, H = rec.n, rec.hs.shape[1], rec.hs.shape[2]
    N = net.nagents
    E = R // N
    dev = rec.hs.device
    mode_avg = getattr(args, 'comm_mode', 'avg') == 'avg'
    mask_zero = bool(args.comm_mask_zero)
    w_cat_t = fc['w_cat_t']
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    c_wt = [m.weight.detach().t().contiguous() for m in net.C_modules]    # per pass C_i^T (H, H)
    dbias = [(m.bias - net.C_modules[0].bias).detach() for m in net.C_modules]
    xh = [z(R, 2 * H) for _ in range(P)]
    comm = [z(E, N, H) for _ in range(P)]
    cs = [z(R, H) for _ in range(P)]
    enc, gates, dgates, dxh = z(R, H), z(R, 4 * H), z(R, 4 * H), z(R, 2 * H)
    dcomm, dcomm_b, dh, denc = z(R, H), z(E, N, H), z(R, H), z(R, H)
    bias_parts, bsum = z(ops.LSTM_BWD_MAX_PARTIALS, 4 * H), z(4 * H)
    dinp = dxh[:, :H]
    dh_rec = torch.zeros((R, H), dtype=torch.float32, device=dev)
    dc_rec = torch.zeros((R, H), dtype=torch.float32, device=dev)
    cuts = _Cuts(args, rec, T, E, N, dev)
    cuts.carry_in(carry, dh_rec, dc_rec)
    h_out = cuts.h_out(rec)
    for t in reversed(range(T)):
        cuts.cut(t, dh_rec, dc_rec)
        alive, gate = cuts.masks(t, rec.alive[t], rec.gate[t])
        # ---- forward: enc (+ encoder.bias + C_0.bias), then the passes
        raw.encode_at(rec.snaps[t], fc['wt'], fc['enc_bias'], out=enc, loc_table=fc['loc_table'])
        h_in, c_in = cuts.entering(t, rec.hs[t], rec.cs[t])
        xh[0][:, H:].copy_(h_in)
        cs[0].copy_(c_in)
        for i in range(P):
            inp_i = xh[i][:, :H]
            torch.add(enc, dbias[i], out=inp_i) if i else inp_i.copy_(enc)
            if mask_zero:
                comm[i].zero_()
            else:
                ops.comm_masked_mean_raw(xh[i].view(E, N, 2 * H)[:, :, H:], alive, gate, mode_avg, True, out=comm[i])
                inp_i.addmm_(comm[i].view(R, H), c_wt[i])
            if i + 1 < P:
                torch.addmm(fc['b_cat'], xh[i], w_cat_t, out=gates)
                cs[i + 1].copy_(cs[i])
                ops.lstm_cell_(gates, cs[i + 1], xh[i + 1][:, H:])
        # ---- backward: heads on the last pass's h, then the passes in reverse
        d = d_out[t]
        torch.addmm(dh_rec, d, fc['w_heads'], out=dh)
        acc['w_heads'].addmm_(d.t(), h_out[t])
        acc['b_heads'].add_(d.sum(0))
        denc.zero_()
        for i in reversed(range(P)):
            torch.addmm(fc['b_cat'], xh[i], w_cat_t, out=gates)
            parts = ops.lstm_cell_backward(gates, cs[i], dh, dc_rec, dgates, dc_rec, bias_parts)   # dc_rec <- dL/dc_i
            torch.sum(parts, 0, out=bsum)
            acc['b_cat'].add_(bsum)
            acc['w_cat_t'].addmm_(xh[i].t(), dgates)
            torch.mm(dgates, w_cat_t.t(), out=dxh)
            denc.add_(dinp)
            acc['c_b'][i].add_(dinp.sum(0))
            if not mask_zero:
                acc['c_w_p'][i].addmm_(dinp.t(), comm[i].view(R, H))
                torch.mm(dinp, c_wt[i].t(), out=dcomm)
                ops.comm_masked_mean_raw(dcomm.view(E, N, H), alive, gate, mode_avg, True, out=dcomm_b)
                torch.add(dxh[:, H:], dcomm_b.view(R, H), out=dh)         # dL/dh_i: what pass i - 1 (or step t - 1) receives
            else:
                dh.copy_(dxh[:, H:])
        dh_rec.copy_(dh)
        dwt, db = raw.encode_backward(denc, rec.snaps[t], want_bias=True)
        acc['wt'].add_(dwt)
        acc['enc_bias'].add_(db)
    return (dh_rec, dc_rec)


MULTIPASS_WINDOW_DEFAULT = True       # args.multipass_window_backward where the flag is absent (main.py carries the same default)
MULTIPASS_WINDOW_COLLECTION_DEFAULT = False     # args.multipass_window_collection likewise: collection-mode windows keep the loop


def _multipass_ring_floats(H, P, collection=False, recorded=False):
    """Floats per row of one chunk step of _backward_window_multipass: per pass the gate record 4H, the inp rows, h and c H each and
    the dxh ring 2H; slot 0 of the h ring and the encoder ring H each; collection mode: slot 0 of a c ring too (the copy of the
    entering c with the starting envs' rows zeroed).  recorded (the passes' record of the window launch stands in for the
    re-evaluation): the dxh ring alone, and in collection mode the two copies of the entering state."""
    if recorded:
        return P * 2 * H + (2 * H if collection else 0)
    return P * (8 * H + ops.record_xh_width(H)) + (3 if collection else 2) * H


def _multipass_chunk_steps(dev, T, R, H, P, most=0, collection=False, recorded=False):
    """Whole steps per chunk of _backward_window_multipass — the largest count for which every launch stays inside its 32-bit limits
    (a chunk's rows x 4H floats below 4 GB: the recording forward and the gate launch's buffer offsets; rows below 2^31 - 2^16: the
    encoder's window stage) and the chunk's rings inside what _ring_fits grants; at most `most` when that is > 0; 0: not even one."""
    tc = min(T, (2 ** 32 - 1) // (R * 4 * H * 4), (2 ** 31 - 2 ** 16 - 1) // R)
    if dev.type == 'cuda':
        tc = min(tc, (device_room(dev) // 4) // (R * _multipass_ring_floats(H, P, collection, recorded) * 4))
    return max(min(tc, most) if most > 0 else tc, 0)


def _multipass_window_ok(args, net, raw, rec, d_out):
    """The recurrent LSTM policy with comm_passes > 1 on a window: hid_size 64 / 128 / 256 (a zero-padded twin at the twin's
    size), at most 16 output columns, the split planes of both directions in the fused cache, the native loop and
    args.multipass_window_backward on, the library's answer for this env (the encoder backward's window form) and room for at least
    one step's rings: _backward_window_multipass.  A collection-mode window (rec.stream) needs args.multipass_window_collection as
    well, which is off where the flag is absent: such a window then keeps the per-step loop."""
    if not rec.recurrent or rec.n < 1 or d_out.shape[-1] > 16 or not d_out.is_cuda:
        return False
    if rec.stream is not None and not bool(getattr(args, 'multipass_window_collection', MULTIPASS_WINDOW_COLLECTION_DEFAULT)):
        return False
    if not bool(getattr(args, 'bptt_native_loop', True)) or not bool(getattr(args, 'multipass_window_backward', MULTIPASS_WINDOW_DEFAULT)):
        return False
    H, N = rec.hs.shape[2], net.nagents
    if H not in (64, 128, 256) or net.hid_size != H or N > 64 or not hasattr(net, 'f_module') or not hasattr(raw, '_h'):
        return False
    fc = net._fused_cache()
    if fc.get('ps_l_wp3') is None or fc.get('ps_l_wp3_bwd') is None or fc.get('ps_c_wp') is None:
        return False
    if not _enc_window(args, raw, H) or not ops.bptt_passes_backward_supported(raw, H, net.comm_passes):
        return False
    return _multipass_chunk_steps(rec.hs.device, rec.n, rec.hs.shape[1], H, net.comm_passes, collection=rec.stream is not None,
                                  recorded=_passes_recorded(net, rec)) >= 1


def _passes_recorded(net, rec):
    """The window launch recorded every pass of every step of this record (EpisodeRecord.pass_*, args.window_record_passes): a
    complete record at the policy's own width — hid 64 / 128, 2..4 passes.  Anything less (a window the library refused, a per-step
    fallback, an allocation that failed) and the backward re-evaluates the passes as ever."""
    if getattr(rec, 'pass_gates', None) is None or rec.pass_inp is None or rec.pass_h is None or rec.pass_c is None:
        return False
    P, H = net.comm_passes, rec.hs.shape[2]
    return rec.n >= 1 and rec.pass_n == rec.n and 2 <= P <= 4 and H in (64, 128) and net.hid_size == H \
        and rec.pass_gates.shape[0] == P and rec.pass_gates.shape[1] >= rec.n


def _backward_window_multipass(args, net, raw, rec, d_out, acc, carry=None, max_chunk_steps=0, dgates_out=None):
    """_backward_episode_multipass for a window on HIP launches alone.  (h, c) entering every step is recorded, so the inner
    passes of all steps are independent of each other: the window is walked in chunks of whole steps, last chunk first, and per chunk
      Tc x raw.encode_at              encoder(obs) + encoder.bias + C_0.bias of every snapshot into a ring
      P x ops.policy_forward_record   pass i over the Tc x E stacked envs, slot i of the (h, c) ring -> slot i + 1 (slot 0: the record's
                                      hs / cs), its activated gates and inp rows kept; C_i.bias - C_0.bias added inside the launch
      ops.bptt_passes_backward        per (step, pass), last first: the cell's derivative in place on the gate record + the input
                                      gradient, the communication backward; the encoder's window stage once per pass behind the loop
      ops.lstm_weight_grad            [W_ih | W_hh]'s gradient over the chunk's P x Tc x R rows, added
    dh / dc carry from chunk to chunk; the heads' gradient is one pass over the window beside the chain.  Behind the chunks: one
    encoder finish, the bias partials of all passes, each pass's dC_i partials, and C_i.bias's gradient read off pass i's bias
    partials — the column sum of pass i's d inp is (the column sum of its dgates) . W_ih.  max_chunk_steps > 0 bounds the chunk (tests); dgates_out (P, T, R, 4H) receives every chunk's dgates (tests).
    Collection mode (rec.stream; `carry` = (dL/dh, dL/dc) from the later window, the pair leaving the first slot is returned): the
    cuts of _Cuts ride inside the same launches.  keep[t] scales what leaves slot t — the chunk's rows go to the call as row_keep,
    the row of the slot in front of the chunk as keep_before, and dh is scaled by keep[T - 1] where it enters the window.  An env
    that starts an episode at slot t has nobody dead and everyone gated off in every pass of that step (masks_window) and zeros
    entering pass 0: slot 0 of the h ring and of a c ring hold the recorded rows times `live`, once per chunk over all its steps
    (the record itself is left alone: the heads' pass beside the chain reads it).
    A window whose launch recorded its passes (_passes_recorded: args.window_record_passes) skips the first two lines and the copy
    into slot 0 of the h ring: per chunk the call is handed slices of the record — pass 0 enters on rec.hs / rec.cs (collection mode:
    the live-scaled copies), pass i >= 1 on rec.pass_h[i - 1] / rec.pass_c[i - 1], the gates are rec.pass_gates[i][t0:t1], overwritten
    by dgates in place — and the weight gradient runs per pass on those slices (they are not one block).  These are the values the
    rollout's cells used; the re-evaluation rounds pass i > 0's encoder bias differently (encoder.bias + C_0.bias, then
    C_i.bias - C_0.bias on top, where the rollout gathers with encoder.bias + C_i.bias).  Counted in net.multipass_recorded_windows."""
    fc = net._fused_cache()
    P = net.comm_passes
    T, R, H = rec.n, rec.hs.shape[1], rec.hs.shape[2]
    N = net.nagents
    E = R // N
    dev = rec.hs.device
    mode_avg = getattr(args, 'comm_mode', 'avg') == 'avg'
    mask_zero = bool(args.comm_mask_zero)
    heads = args.naction_heads
    cuts = _Cuts(args, rec, T, E, N, dev)                         # (lock-step: the detach points; collection: row factors, masks, carry)
    assert cuts.on or carry is None, "a carried gradient would be dropped: only collection-mode windows (rec.stream) take a carry"
    recorded = _passes_recorded(net, rec)
    Tc = _multipass_chunk_steps(dev, T, R, H, P, max_chunk_steps, collection=cuts.on, recorded=recorded)
    assert Tc >= 1, "no room for one step's rings (_multipass_window_ok answers first)"
    xw = ops.record_xh_width(H)
    empty = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    zeros = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
    if recorded:                                                  # (the record stands in for every ring but dxh's)
        enc = gates = inp = cring = None
        hring = empty(1, Tc, R, H) if cuts.on else None           # collection: h ENTERING pass 0, the starting envs' rows zeroed
    else:
        enc, gates, inp = empty(Tc, R, H), empty(P, Tc, R, 4 * H), empty(P, Tc, R, xw)
        hring, cring = empty(P + 1, Tc, R, H), empty(P, Tc, R, H)                               # cring[i]: c LEAVING pass i
    dxh = empty(P, Tc, R, 2 * H)
    c_in = empty(Tc, R, H) if cuts.on else None                   # collection: c ENTERING pass 0, the starting envs' rows zeroed
    dh_rec, dc_rec = zeros(R, H), zeros(R, H)
    cuts.carry_in(carry, dh_rec, dc_rec, at_border=True)
    alive_w, gate_w = cuts.masks_window(rec.alive[:T], rec.gate[:T], fill_gate=False)
    bias_parts = zeros(P, (R + 63) // 64, 4 * H)
    dcw_parts = None if mask_zero else zeros(P, ops.comm_backward_partials(E, N), H, H)
    c_weights = None if mask_zero else [m.weight.detach() for m in net.C_modules]
    dhead = _dhead_rows(d_out, T)
    work = acc.setdefault('_work', {})

    def stacked(ms):                                              # Tn entries (E, N) or None -> (Tn x E, N), None: everyone
        if all(m is None for m in ms):
            return None
        ones = next(m for m in ms if m is not None).new_ones((E, N))
        return torch.stack([m if m is not None else ones for m in ms]).contiguous()
    with _heads_grad_beside(args, rec, d_out, acc, T, R, H):
        first = True
        for t1 in range(T, 0, -Tc):
            t0 = max(t1 - Tc, 0)
            Tn = t1 - t0
            alive, gate = alive_w[t0:t1], gate_w[t0:t1]
            if cuts.on:
                torch.mul(rec.hs[t0:t1], cuts.live_rows[t0:t1], out=hring[0, :Tn])
                torch.mul(rec.cs[t0:t1], cuts.live_rows[t0:t1], out=c_in[:Tn])
            elif not recorded:
                hring[0, :Tn].copy_(rec.hs[t0:t1])
            if recorded:
                g_p = [rec.pass_gates[i, t0:t1] for i in range(P)]
                x_p = [rec.pass_inp[i, t0:t1] for i in range(P)]
                h_p = [hring[0, :Tn] if cuts.on else rec.hs[t0:t1]] + [rec.pass_h[i, t0:t1] for i in range(P - 1)]
                cs = [c_in[:Tn] if cuts.on else rec.cs[t0:t1]] + [rec.pass_c[i, t0:t1] for i in range(P - 1)]
            else:
                for k in range(Tn):
                    raw.encode_at(rec.snaps[t0 + k], fc['wt'], fc['enc_bias'], out=enc[k], loc_table=fc['loc_table'])
                alive_st, gate_st = stacked(alive), stacked(gate)
                g_p, x_p, h_p = [gates[i, :Tn] for i in range(P)], [inp[i, :Tn] for i in range(P)], [hring[i, :Tn] for i in range(P)]
                cs = [c_in[:Tn] if cuts.on else rec.cs[t0:t1]] + [cring[i, :Tn] for i in range(P - 1)]
            for i in range(0 if recorded else P):
                ops.policy_forward_record(fc, H, heads, mode_avg, mask_zero, enc[:Tn].view(Tn * R, H), Tn * E, N,
                                          hring[i, :Tn].view(Tn * R, H), cs[i].reshape(Tn * R, H), hring[i + 1, :Tn].view(Tn * R, H),
                                          cring[i, :Tn].view(Tn * R, H), alive_st, gate_st, gates[i, :Tn].view(Tn * R, 4 * H),
                                          inp[i, :Tn].view(Tn * R, xw), pass_index=i, enc_add=fc.get('enc_dbias_p%d' % i) if i else None)
            ops.bptt_passes_backward(raw, Tn, E, N, H, g_p, h_p, cs,
                                     dhead[t0:t1], rec.snaps[t0:t1], alive, gate, fc['ps_l_wp3_bwd'], fc['w_heads'], c_weights, dh_rec,
                                     dc_rec, [dxh[i, :Tn] for i in range(P)], [bias_parts[i] for i in range(P)],
                                     None if mask_zero else [dcw_parts[i] for i in range(P)], mode_avg=mode_avg, comm_zero=mask_zero,
                                     detach_gap=cuts.gap, t_first=t0, enc_first=first,
                                     row_keep=cuts.keep_flat[t0:t1] if cuts.on else None,
                                     keep_before=cuts.keep_flat[t0 - 1] if cuts.on and t0 > 0 else None)
            first = False
            if dgates_out is not None:
                for i in range(P):
                    dgates_out[i, t0:t1].copy_(g_p[i])
            split = bool(getattr(args, 'gate_split', True))
            if recorded:                                          # (the record's slices of a chunk are not one block)
                for i in range(P):
                    ops.lstm_weight_grad(x_p[i], h_p[i], g_p[i], acc['w_cat_t'], accumulate=True, work=work, split=split)
            elif Tn == Tc:                                        # the chunk's P x Tc x R rows in one launch
                ops.lstm_weight_grad(inp, hring[:P], gates, acc['w_cat_t'], accumulate=True, work=work, split=split)
            else:                                                 # (a short last chunk: the passes' rows are not one block)
                for i in range(P):
                    ops.lstm_weight_grad(inp[i, :Tn], hring[i, :Tn], gates[i, :Tn], acc['w_cat_t'], accumulate=True, work=work, split=split)
        dwt, db = raw.encode_backward_window_finish(H, want_bias=True)
        acc['wt'].add_(dwt)
        acc['enc_bias'].add_(db)
        bsum = bias_parts.sum(1)                                  # (P, 4H): the column sums of every pass's dgates
        acc['b_cat'].add_(bsum.sum(0))
        w_ih_t = fc['w_cat_t'][:H]                                # (H, 4H) = W_ih^T
        for i in range(P):
            acc['c_b'][i].add_(torch.mv(w_ih_t, bsum[i]))
            if not mask_zero:
                acc['c_w_p'][i].add_(dcw_parts[i].sum(0))
    net.multipass_window_backwards = getattr(net, 'multipass_window_backwards', 0) + 1
    if recorded:
        net.multipass_recorded_windows = getattr(net, 'multipass_recorded_windows', 0) + 1
        rec.pass_n = 0                                            # (pass_gates holds dgates now)
    net.multipass_window_chunk = Tc
    return (dh_rec, dc_rec)


def _backward_episode_commnet(args, net, raw, rec, d_out, acc):
    """The NON-recurrent module (comm.py:127-129,179-205,220-224):  x = tanh(encoder(obs));  h_0 = x;
    h_{i+1} = tanh(x + f_i(h_i) + C_i(comm(h_i)));  [logits | value] = W_heads h_P + b.  No state crosses a step, so every
    recorded step is differentiated on its own: the forward is re-evaluated from the env snapshot (sparse encoder, the masked
    mean, library GEMMs for the H x H layers), then
        dz_i = dh_{i+1} (1 - h_{i+1}^2);   dx += dz_i;   dF_i += dz_i^T h_i;   dC_i += dz_i^T comm_i;
        dh_i = dz_i F_i + mix(dz_i C_i)            (the mixing matrix of the communication block is symmetric)
    and finally d enc = (dx + dh_0)(1 - x^2) through ic3_env_encode_backward on the snapshot.  A record that qualifies
    (_commnet_window_ok) goes to _backward_window_commnet — the same arithmetic as window-wide launches — instead of the loop below,
    as _backward_episode_baseline hands its own over to _backward_window_mlp."""
    if _commnet_window_ok(args, net, raw, rec, d_out):
        return _backward_window_commnet(args, net, raw, rec, d_out, acc)
    cn = net._commnet_cache()
    P = net.comm_passes
    T, R, H = rec.n, rec.rows, net.hid_size
    N = net.nagents
    E = R // N
    dev = rec.device
    mode_avg = getattr(args, 'comm_mode', 'avg') == 'avg'
    mask_zero = bool(args.comm_mask_zero)
    z = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    Cw = [m.weight.detach() for m in net.C_modules]               # (H, H): y = v C^T
    Fw = [m.weight.detach() for m in net.f_modules]
    bias = cn['bias']                                             # (P, H) = C_i.bias + f_i.bias
    enc = z(R, H)
    hs = [z(R, H) for _ in range(P + 1)]
    x = hs[0]                                                     # h_0 = x = tanh(encoder(obs))
    comm = [z(E, N, H) for _ in range(P)]
    dz, dh, dx, tmp, mixed = z(R, H), z(R, H), z(R, H), z(R, H), z(E, N, H)
    w_heads = cn['w_heads']
    tanh_bwd = torch.ops.aten.tanh_backward.grad_input            # grad (1 - out^2) in one launch
    fgrad = [_RowBlockGrad(acc['f_w'][i], R, 32) for i in range(P)]                                  # dz_i^T . h_i
    cgrad = [None if mask_zero else _RowBlockGrad(acc['c_w_p'][i], R, 32) for i in range(P)]         # dz_i^T . comm_i
    enc_grad = _EncoderGrad(raw, acc, 'wt', 'enc_bias')
    cuts = _Cuts(args, rec, T, E, N, dev)  # collection mode: no state crosses a step — only the masks of an env that starts an episode
    for t in reversed(range(T)):
        alive, gate = cuts.masks(t, rec.alive[t], rec.gate[t])
        # ---- forward of step t again
        raw.encode_at(rec.snaps[t], cn['wt'], cn['enc_bias'], out=enc, loc_table=cn['loc_table'])
        torch.tanh(enc, out=x)
        for i in range(P):
            if mask_zero:
                comm[i].zero_()
            else:
                ops.comm_masked_mean_raw(hs[i].view(E, N, H), alive, gate, mode_avg, True, out=comm[i])
            torch.add(x, bias[i], out=tmp)                        # x + both biases
            tmp.addmm_(hs[i], Fw[i].t())                          # + f_i(h_i)
            if not mask_zero:
                tmp.addmm_(comm[i].view(R, H), Cw[i].t())         # + C_i(comm_i)
            torch.tanh(tmp, out=hs[i + 1])
        # ---- backward: heads, then the passes last to first
        d = d_out[t]
        acc['w_heads'].addmm_(d.t(), hs[P])
        acc['b_heads'].add_(d.sum(0))
        torch.mm(d, w_heads, out=dh)
        for i in reversed(range(P)):
            tanh_bwd(dh, hs[i + 1], grad_input=dz)                # dh (1 - h^2)
            if i == P - 1:
                dx.copy_(dz)
            else:
                dx.add_(dz)
            fgrad[i].add(dz, hs[i])
            acc['cf_b'][i].add_(dz.sum(0))
            torch.mm(dz, Fw[i], out=dh)
            if not mask_zero:
                cgrad[i].add(dz, comm[i].view(R, H))
                torch.mm(dz, Cw[i], out=tmp)
                # dh += mix(dz C_i): the mixing matrix is symmetric — the same kernel on the gradient, the addend along
                ops.comm_masked_mean_raw(tmp.view(E, N, H), alive, gate, mode_avg, True, out=mixed, addend=dh)
                dh, mixed = mixed.view(R, H), dh.view(E, N, H)
        dx.add_(dh)                                               # h_0 = x
        tanh_bwd(dx, x, grad_input=tmp)                           # through x = tanh(enc)
        enc_grad.step(tmp, rec.snaps[t])
    enc_grad.finish(H)
    for i in range(P):
        fgrad[i].finish()
        if cgrad[i] is not None:
            cgrad[i].finish()


COMMNET_WINDOW_SIZES = (64, 128, 256)     # ic3_commnet_backward


def _commnet_window_ok(args, net, raw, rec, d_out):
    """The non-recurrent CommNet module (`supported` has tied it to its own env) at hid_size 64 / 128 / 256 — a zero-padded twin at
    the twin's size —, at most 16 output columns, the native loop (args.bptt_native_loop) and args.commnet_window_backward on, the
    library's answer for this env and the room for what ops.commnet_backward allocates: with Q = T x R rows (a chunk's, when the
    library splits the window) the enc / h_pass ring of (P + 1) Q H floats, dxh Q 2H, dz, dx, de and dh Q H each — (P + 7) Q H
    floats — plus the partials' scratch (ops.commnet_backward_ring_floats): _backward_window_commnet."""
    H, T = net.hid_size, rec.n
    if rec.recurrent or H not in COMMNET_WINDOW_SIZES or T < 1 or d_out.shape[-1] > 16 or not d_out.is_cuda:
        return False
    if not bool(getattr(args, 'bptt_native_loop', True)) or not bool(getattr(args, 'commnet_window_backward', True)):
        return False
    N = net.nagents
    if not hasattr(raw, '_h') or not ops.commnet_backward_supported(raw, H, N):
        return False
    chunk = int(getattr(args, 'commnet_window_chunk_steps', 0))
    return _ring_fits(rec.device, 4 * ops.commnet_backward_ring_floats(raw, T, rec.rows // N, N, H, net.comm_passes, chunk))


def _backward_window_commnet(args, net, raw, rec, d_out, acc):
    """_backward_episode_commnet for a whole window through ic3_commnet_backward (csrc/bptt_kernels.hip).  No state crosses a step,
    so the window is T x R independent rows in T x E independent envs: enc of every snapshot into a ring (T encoder launches), the
    forward again over all T x E envs in one launch with h_0 .. h_P kept, then per pass, last to first, three window-wide launches
    — dz_i = dh_{i+1} (1 - h_{i+1}^2) with dz_i F_i beside it, the communication backward (dh_i = dz_i F_i + mix(dz_i) C_i and
    dC_i = mix(dz_i)^T h_i: the mixing matrix is symmetric), dF_i = dz_i^T h_i — and fixed-order sums of the partials; de = (sum_i
    dz_i + dh_0)(1 - h_0^2), the sparse encoder's first stage over the de ring, the heads' gradient on the recomputed h_P.  All on
    the current stream, inside the one host call (the heads' pass reads a ring that exists only there: no second stream, nothing to
    join).  Collection mode needs only the masks of the envs that start an episode (cuts.masks_window); the record is read, never
    written.  args.commnet_window_chunk_steps > 0 bounds the steps per chunk (tests)."""
    cn = net._commnet_cache()
    T, R, H, N = rec.n, rec.rows, net.hid_size, net.nagents
    E = R // N
    dev = rec.device
    mask_zero = bool(args.comm_mask_zero)
    cuts = _Cuts(args, rec, T, E, N, dev)
    alive, gate = cuts.masks_window(rec.alive[:T], rec.gate[:T])
    if all(m is None for m in rec.gate[:T]):                      # no gate head: an env that starts an episode talks, as in the
        gate = [None] * T                                         # step launch and in the loop (cuts.masks without fill_gate)

    def stacked(ms):                                           # T entries (E, N) or None -> (T, E, N), None: everyone
        if all(m is None for m in ms):
            return None
        ones = next(m for m in ms if m is not None).new_ones((E, N))
        return torch.stack([m if m is not None else ones for m in ms]).contiguous()
    enc_window = _enc_window(args, raw, H)
    ops.commnet_backward(raw, T, E, N, H, _dhead_rows(d_out, T), rec.snaps, stacked(alive), stacked(gate), cn['wt'], cn['enc_bias'],
                         cn['wp'], cn['bias'], cn['w_heads'], [m.weight.detach() for m in net.f_modules],
                         [m.weight.detach() for m in net.C_modules], acc['f_w'], acc['c_w_p'], acc['cf_b'],
                         heads_w_grad=acc['w_heads'], heads_b_grad=acc['b_heads'], wp3=cn.get('wp3'), loc_table=cn['loc_table'],
                         mode_avg=getattr(args, 'comm_mode', 'avg') == 'avg', comm_zero=mask_zero, enc_first=True,
                         enc_window=enc_window, max_chunk_steps=int(getattr(args, 'commnet_window_chunk_steps', 0)),
                         work=acc.setdefault('_work', {}))
    # (the ordered finish where the env has the window form: the encoder's gradient identical run to run, like the rest of the path)
    dwt, db = raw.encode_backward_window_finish_ordered(H, want_bias=True) if enc_window \
        else raw.encode_backward_finish(H, want_bias=True)
    acc['wt'].add_(dwt)
    acc['enc_bias'].add_(db)
    net.commnet_window_backwards = getattr(net, 'commnet_window_backwards', 0) + 1


def standin_for_backward(args, net, rec=None):
    """models.RNN with the LSTM cell IS the recurrent CommNet policy with the communication block off (models._KernelStandIn): where
    that stand-in runs at the baseline's own hidden size with the fused gate launches (hid 64 / 128 / 256), its backward is
    backward_episode on the stand-in — gate launch with the input gradient, recorded gates when the rollout stored them —
    instead of the library chain of _backward_episode_baseline.  Returns the stand-in module, or None."""
    if not (getattr(args, 'recurrent', False) and getattr(args, 'rnn_type', 'MLP') == 'LSTM') or not hasattr(net, 'lstm_unit'):
        return None
    if not bool(getattr(args, 'baseline_fused_backward', True)):
        return None
    sk = getattr(net, '_stand_in', None)
    if sk is None or ops.padded_hidden(args.hid_size) is not None or not ops.lstm_gates_backward_supported(args.hid_size):
        return None
    if rec is not None and (not rec.recurrent or rec.hs.shape[2] != args.hid_size):
        return None
    with torch.no_grad():
        si = sk.get()
        if si is None or si._fused_cache().get('ps_l_wp') is None:
            return None
    return si


def _backward_episode_standin(net, si, raw, rec, d_out, acc, carry=None):
    """IRIC (models.RNN, LSTM) through the stand-in's backward; its accumulators are folded into the baseline's by name:
    encoder = affine1, [W_ih | W_hh] / b_ih + b_hh = lstm_unit's, heads; C (all zeros, never read: comm_mask_zero) has none."""
    acc2 = acc.get('_standin')
    if acc2 is None:
        acc2 = acc['_standin'] = new_accumulators(si)
    walks = getattr(si, 'lstm_backward_walks', 0)
    out = backward_episode(si.args, si, raw, rec, d_out, acc2, carry=carry)
    # (args.backward_walk_lstm: the windows walked in one launch are counted on the policy the trainer holds)
    net.lstm_backward_walks = getattr(net, 'lstm_backward_walks', 0) + getattr(si, 'lstm_backward_walks', 0) - walks
    return out


def fold_standin(acc):
    """(behind the last episode of the batch) the stand-in's accumulators -> the baseline's"""
    acc2 = acc.pop('_standin', None)
    if acc2 is None:
        return
    H = acc['l_b'].shape[0] // 4
    acc['wt'].add_(acc2['wt'])
    acc['a1_b'].add_(acc2['enc_bias'])
    acc['l_w_ih'].add_(acc2['w_cat_t'][:H].t())
    acc['l_w_hh'].add_(acc2['w_cat_t'][H:].t())
    acc['l_b'].add_(acc2['b_cat'])
    acc['w_heads'].add_(acc2['w_heads'])
    acc['b_heads'].add_(acc2['b_heads'])


RNN_WINDOW_SIZES = (64, 128, 256)     # ic3_rnn_backward_wide


def _rnn_window_ok(args, net, raw, rec, d_out):
    """models.RNN with the tanh recurrence on a record at its own hid_size (64 / 128 / 256), at most 16 output columns, the native loop
    on (args.bptt_native_loop), the library's answer and the room for the T x R x H ring of dz: _backward_window_rnn."""
    H = args.hid_size
    if not rec.recurrent or getattr(args, 'rnn_type', 'MLP') != 'MLP' or not hasattr(net, 'affine2') or H not in RNN_WINDOW_SIZES:
        return False
    if rec.hs.shape[2] != H or d_out.shape[-1] > 16 or not bool(getattr(args, 'bptt_native_loop', True)) or not rec.hs.is_cuda:
        return False
    if not hasattr(raw, '_h') or not ops.rnn_backward_supported(raw, H):
        return False
    return _ring_fits(rec.hs.device, rec.n * rec.hs.shape[1] * H * 4)


def _backward_window_rnn(args, net, raw, rec, d_out, acc, carry=None):
    """_backward_episode_baseline's tanh branch for a whole window through ic3_rnn_backward_wide (csrc/bptt_kernels.hip; hid 64 / 128 / 256).  Per step, last
    to first, ONE launch: dh_t = dh + d_t . W_heads, dz_t = dh_t (1 - h_t^2) into a ring of T slots, dh <- (dz_t . A2) * keep_{t-1},
    the column sums of dz_t as per-workgroup partials; then the sparse encoder's first stage over the ring, and affine2's weight
    gradient sum_t dz_t^T (live_t h_{t-1}) over all T x R rows in one launch.  Behind it: the encoder's expansion (affine1.weight),
    the partials' sum (both biases: affine1(obs) + affine2(h) share dz), the heads' pass beside the chain.  Same cuts as the loop
    (detach points; collection mode: keep / row_live, the carry in and out); the record is read, never written.
    args.backward_walk: the T launches as ONE (an ic3_rnn_bptt_walk descriptor: every 64-row tile walked last step to first by one
    workgroup, dL/dh on chip) — the same dz, dh and weight gradients bit for bit, the bias partials one row per tile."""
    T, R, H = rec.n, rec.hs.shape[1], rec.hs.shape[2]
    N = net.args.nagents
    E = R // N
    dev = rec.hs.device
    dh = torch.zeros((R, H), dtype=torch.float32, device=dev)
    dz = torch.empty((T, R, H), dtype=torch.float32, device=dev)
    walk = bool(getattr(args, 'backward_walk', 0))
    parts = torch.zeros(((R + 63) // 64 if walk else ops.rnn_backward_partials(R, H), H), dtype=torch.float32, device=dev)
    cuts = _Cuts(args, rec, T, E, N, dev)
    cuts.carry_in(carry, dh, at_border=True)
    dhead = _dhead_rows(d_out, T)
    h_last = None if rec.h_last_is_slot(T) else rec.h_last
    w_heads, a2 = _baseline_w_heads(net), net.affine2.weight.detach().contiguous()
    enc_window = _enc_window(args, raw, H)
    with _heads_grad_beside(args, rec, d_out, acc, T, R, H):
        ops.rnn_backward(raw, T, E, N, H, rec.hs, dhead, rec.snaps, a2, w_heads, dh, dz, parts, h_last=h_last,
                         detach_gap=cuts.gap, row_live=cuts.live_flat, row_keep=cuts.keep_flat, enc_first=True,
                         enc_window=enc_window, a2_grad=acc['a2_w'], work=acc.setdefault('_work', {}), walk=walk)
        dwt, _ = raw.encode_backward_window_finish(H, want_bias=False) if enc_window else raw.encode_backward_finish(H, want_bias=False)
        acc['wt'].add_(dwt)
        bsum = parts.sum(0)
        acc['a1_b'].add_(bsum)
        acc['a2_b'].add_(bsum)
    if walk:
        net.rnn_backward_walks = getattr(net, 'rnn_backward_walks', 0) + 1
    return (dh, dh)


MLP_WINDOW_SIZES = (64, 128, 256)     # ic3_mlp_backward_wide


def mlp_window_wanted(args, net, raw):
    """What a rollout must hold for _backward_window_mlp before it records h_fin: the IC baseline itself (models.MLP, not its
    recurrent subclass) at hid 64 / 128 / 256 — no zero-padded twin —, the native loop on, and the library's answer for this env."""
    from . import models
    H = args.hid_size
    if type(net) is not models.MLP or getattr(args, 'recurrent', False) or H not in MLP_WINDOW_SIZES:
        return False
    if not bool(getattr(args, 'bptt_native_loop', True)) or ops.padded_hidden(H) is not None:
        return False
    return hasattr(raw, '_h') and ops.mlp_backward_supported(raw, H)


def _mlp_window_ok(args, net, raw, rec, d_out):
    """models.MLP on a record whose step launches stored h of every step (h_fin), hid_size 64 / 128 / 256, at most 16 output columns, the
    native loop on (args.bptt_native_loop), the library's answer and the room for the three T x R x H rings (x1, dz, de):
    _backward_window_mlp."""
    if rec.recurrent or not mlp_window_wanted(args, net, raw):
        return False
    H, T = args.hid_size, rec.n
    h = getattr(rec, 'h_fin', None)
    if h is None or T < 1 or rec.h_fin_n != T or h.shape[0] < T or tuple(h.shape[1:]) != (rec.rows, H) or not h.is_cuda:
        return False
    if d_out.shape[-1] > 16:
        return False
    return _ring_fits(h.device, 3 * T * rec.rows * H * 4)


def _backward_window_mlp(args, net, raw, rec, d_out, acc):
    """_backward_episode_baseline's non-recurrent branch for a whole window through ic3_mlp_backward_wide (csrc/bptt_kernels.hip; hid 64 / 128 / 256).  No
    state crosses a step, so the window is T x R independent rows: e of every snapshot into a ring (T encoder launches), then ONE
    launch — x1 = tanh(e) over e, dz = (d . W_heads)(1 - h^2) with the h the step launches recorded (rec.h_fin), de = (dz . A2 +
    dz)(1 - x1^2), the column sums of dz as per-workgroup partials —, the sparse encoder's first stage over the de ring and affine2's
    weight gradient sum dz^T x1 over all rows in one launch.  Behind it: the encoder's expansion (affine1.weight; its bias sum is
    affine1.bias's gradient), the partials' sum (affine2.bias), the heads' pass beside the chain.  Collection mode needs no cuts
    (the loop applies none either); the record is read, never written."""
    T, R, H = rec.n, rec.rows, args.hid_size
    N = net.args.nagents
    E = R // N
    dev = rec.h_fin.device
    x1, dz, de = (torch.empty((T, R, H), dtype=torch.float32, device=dev) for _ in range(3))
    parts = torch.empty((ops.mlp_backward_partials(T * R, H), H), dtype=torch.float32, device=dev)
    dhead = _dhead_rows(d_out, T)
    wt = net.affine1.weight.detach().t().contiguous()
    w_heads, a2 = _baseline_w_heads(net), net.affine2.weight.detach().contiguous()
    enc_window = _enc_window(args, raw, H)
    with _heads_grad_beside(args, rec, d_out, acc, T, R, H):
        ops.mlp_backward(raw, T, E, N, H, rec.h_fin, dhead, rec.snaps, wt, net.affine1.bias.detach().contiguous(), a2, w_heads,
                         x1, dz, de, parts, enc_first=True, enc_window=enc_window, a2_grad=acc['a2_w'],
                         work=acc.setdefault('_work', {}))
        # (the ordered finish: affine1's gradient identical run to run, like everything else on this path — where the env has the
        #  window form; the per-step form's finish adds with float atomics, so there affine1.weight's last bits may move)
        dwt, db = raw.encode_backward_window_finish_ordered(H, want_bias=True) if enc_window \
            else raw.encode_backward_finish(H, want_bias=True)
        acc['wt'].add_(dwt)
        acc['a1_b'].add_(db)
        acc['a2_b'].add_(parts.sum(0))


def _backward_episode_baseline(args, net, raw, rec, d_out, acc, carry=None):
    """The IC / IRIC baselines of models.py:8-97 (no communication), differentiated by hand over the recorded rollout:
      MLP  (models.py:23-34)   x1 = tanh(affine1(obs));  h = tanh(affine2(x1) + x1)         every step on its own
      RNN  (models.py:68-92)   rnn_type 'MLP':  h_t = tanh(affine2(h_{t-1}) + affine1(obs))
                               rnn_type 'LSTM': (h_t, c_t) = LSTMCell(affine1(obs), (h_{t-1}, c_{t-1}))
    heads / value on h.  affine1 is the sparse encoder (ic3_env_encode_at on the step's snapshot, ic3_env_encode_backward);
    the recurrent gradient is cut where the Trainer detaches the hidden state (trainer.py:56-60).  The MLP branch of a record
    that holds h of every step goes to _backward_window_mlp (one launch over the window) instead of the loop below."""
    if not rec.recurrent and _mlp_window_ok(args, net, raw, rec, d_out):
        return _backward_window_mlp(args, net, raw, rec, d_out, acc)
    T, H = rec.n, args.hid_size
    R = rec.rows if not rec.recurrent else rec.hs.shape[1]
    dev = net.affine1.weight.device
    z = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    wt = net.affine1.weight.detach().t().contiguous()
    b1 = net.affine1.bias.detach()
    w_heads = _baseline_w_heads(net)
    enc, dh, dz = z(R, H), z(R, H), z(R, H)
    recurrent = rec.recurrent
    lstm = recurrent and getattr(args, 'rnn_type', 'MLP') == 'LSTM'
    if recurrent:
        dh_rec = torch.zeros((R, H), dtype=torch.float32, device=dev)
    if lstm:
        cell = net.lstm_unit
        w_ih, w_hh = cell.weight_ih.detach(), cell.weight_hh.detach()
        b_cat = (cell.bias_ih + cell.bias_hh).detach()
        gates, dgates = z(R, 4 * H), z(R, 4 * H)
        parts, bsum = z(ops.LSTM_BWD_MAX_PARTIALS, 4 * H), z(4 * H)
        dc_rec = torch.zeros((R, H), dtype=torch.float32, device=dev)
    elif recurrent:
        A2 = net.affine2.weight.detach()
    else:
        A2, b2 = net.affine2.weight.detach(), net.affine2.bias.detach()
        x1, hcur = z(R, H), z(R, H)
    tanh_bwd = torch.ops.aten.tanh_backward.grad_input            # grad (1 - out^2) in one launch
    a2grad = None if lstm else _RowBlockGrad(acc['a2_w'], R, 32)  # dz^T . x1 / dz^T . h_{t-1}
    enc_grad = _EncoderGrad(raw, acc, 'wt', 'a1_b')
    cuts = _Cuts(args, rec, T, R // net.args.nagents, net.args.nagents, dev)
    if recurrent:
        cuts.carry_in(carry, dh_rec, dc_rec if lstm else None)
        h_out = cuts.h_out(rec)
    for t in reversed(range(T)):
        d = d_out[t]
        raw.encode_at(rec.snaps[t], wt, b1, out=enc)              # affine1(obs_t)
        if not recurrent:                                         # ---- MLP
            torch.tanh(enc, out=x1)
            torch.addmm(b2, x1, A2.t(), out=hcur)
            hcur.add_(x1)
            torch.tanh(hcur, out=hcur)
            acc['w_heads'].addmm_(d.t(), hcur)
            acc['b_heads'].add_(d.sum(0))
            torch.mm(d, w_heads, out=dh)
            tanh_bwd(dh, hcur, grad_input=dz)                                     # through the outer tanh
            a2grad.add(dz, x1)
            acc['a2_b'].add_(dz.sum(0))
            torch.addmm(dz, dz, A2, out=dh)                                       # d x1 = dz A2 + dz (the skip)
            tanh_bwd(dh, x1, grad_input=dz)                                       # through x1 = tanh(enc)
        else:
            cuts.cut(t, *((dh_rec, dc_rec) if lstm else (dh_rec,)))          # (h_t, c_t) were handed on detached / the episode ended
            h_prev, c_prev = cuts.entering(t, rec.hs[t], rec.cs[t] if lstm else None)
            h_t = h_out[t]
            acc['w_heads'].addmm_(d.t(), h_t)
            acc['b_heads'].add_(d.sum(0))
            torch.addmm(dh_rec, d, w_heads, out=dh)
            if lstm:                                              # ---- RNN, LSTM cell
                torch.addmm(b_cat, enc, w_ih.t(), out=gates)
                gates.addmm_(h_prev, w_hh.t())
                p_ = ops.lstm_cell_backward(gates, c_prev, dh, dc_rec, dgates, dc_rec, parts)   # dc_rec <- dL/dc_{t-1}
                torch.sum(p_, 0, out=bsum)
                acc['l_b'].add_(bsum)
                acc['l_w_ih'].addmm_(dgates.t(), enc)
                acc['l_w_hh'].addmm_(dgates.t(), h_prev)
                torch.mm(dgates, w_ih, out=dz)                    # d enc
                torch.mm(dgates, w_hh, out=dh_rec)                # dL/dh_{t-1}
            else:                                                 # ---- RNN, tanh recurrence
                tanh_bwd(dh, h_t, grad_input=dz)
                a2grad.add(dz, h_prev)
                acc['a2_b'].add_(dz.sum(0))
                torch.mm(dz, A2, out=dh_rec)
        enc_grad.step(dz, rec.snaps[t])
    enc_grad.finish(H)
    if a2grad is not None:
        a2grad.finish()
    if recurrent:
        return (dh_rec, dc_rec if lstm else dh_rec)


def new_accumulators(net):
    if _is_baseline(net):
        H, dev = net.args.hid_size, net.affine1.weight.device
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
        OT = sum(hd.weight.shape[0] for hd in net.heads) + 1
        acc = dict(wt=z(net.affine1.weight.shape[1], H), a1_b=z(H), w_heads=z(OT, H), b_heads=z(OT), baseline=True)
        if hasattr(net, 'lstm_unit'):
            acc.update(l_w_ih=z(4 * H, H), l_w_hh=z(4 * H, H), l_b=z(4 * H))
        else:
            acc.update(a2_w=z(H, H), a2_b=z(H))
        return acc
    if not getattr(net.args, 'recurrent', False):                 # the non-recurrent module
        cn = net._commnet_cache()
        H, P, dev = net.hid_size, net.comm_passes, cn['wt'].device
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
        return dict(wt=z(*cn['wt'].shape), enc_bias=z(H), w_heads=z(*cn['w_heads'].shape), b_heads=z(cn['b_heads'].shape[0]),
                    c_w_p=[z(H, H) for _ in range(P)], f_w=[z(H, H) for _ in range(P)], cf_b=[z(H) for _ in range(P)])
    fc = net._fused_cache()
    H = net.hid_size
    dev = fc['wt'].device
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    acc = dict(wt=z(*fc['wt'].shape), enc_bias=z(H), c_w=z(H, H), w_cat_t=z(2 * H, 4 * H), b_cat=z(4 * H),
               w_heads=z(*fc['w_heads'].shape), b_heads=z(fc['b_heads'].shape[0]))
    if net.comm_passes > 1:                                               # per pass: C_i.weight, C_i.bias
        acc['c_w_p'] = [z(H, H) for _ in range(net.comm_passes)]
        acc['c_b'] = [z(H) for _ in range(net.comm_passes)]
    return acc


def assign_grads(net, acc):
    """accumulators -> .grad of the reference's parameters (state_dict names of comm.py)."""
    def put(p, g):
        p.grad = g.reshape(p.shape).contiguous()
    if acc.get('baseline'):                                       # models.MLP / models.RNN
        fold_standin(acc)
        put(net.affine1.weight, acc['wt'].t())
        put(net.affine1.bias, acc['a1_b'])
        if 'l_b' in acc:
            put(net.lstm_unit.weight_ih, acc['l_w_ih'])
            put(net.lstm_unit.weight_hh, acc['l_w_hh'])
            put(net.lstm_unit.bias_ih, acc['l_b'].clone())
            put(net.lstm_unit.bias_hh, acc['l_b'].clone())
        else:
            put(net.affine2.weight, acc['a2_w'])
            put(net.affine2.bias, acc['a2_b'])
        off = 0
        for hd in net.heads:
            A = hd.weight.shape[0]
            put(hd.weight, acc['w_heads'][off:off + A])
            put(hd.bias, acc['b_heads'][off:off + A])
            off += A
        put(net.value_head.weight, acc['w_heads'][off:off + 1])
        put(net.value_head.bias, acc['b_heads'][off:off + 1])
        return
    put(net.encoder.weight, acc['wt'].t())
    put(net.encoder.bias, acc['enc_bias'].clone())
    if 'f_w' in acc:                                              # the non-recurrent module: C_i, f_i per pass (+ shared modules)
        done = {}
        for mods, wkey in ((net.C_modules, 'c_w_p'), (net.f_modules, 'f_w')):
            for i, m in enumerate(mods):
                if id(m) in done:                                 # share_weights: one module, the passes' sums
                    m.weight.grad.add_(acc[wkey][i])
                    m.bias.grad.add_(acc['cf_b'][i])
                else:
                    put(m.weight, acc[wkey][i].clone())
                    put(m.bias, acc['cf_b'][i].clone())
                    done[id(m)] = True
        off = 0
        for hd in net.heads:
            A = hd.weight.shape[0]
            put(hd.weight, acc['w_heads'][off:off + A])
            put(hd.bias, acc['b_heads'][off:off + A])
            off += A
        put(net.value_head.weight, acc['w_heads'][off:off + 1])
        put(net.value_head.bias, acc['b_heads'][off:off + 1])
        return
    if net.comm_passes > 1:
        done = {}
        for i, m in enumerate(net.C_modules):                             # share_weights: one module, the passes' sums
            if id(m) in done:
                m.weight.grad.add_(acc['c_w_p'][i])
                m.bias.grad.add_(acc['c_b'][i])
            else:
                put(m.weight, acc['c_w_p'][i].clone())
                put(m.bias, acc['c_b'][i].clone())
                done[id(m)] = True
    else:
        put(net.C_modules[0].weight, acc['c_w'])
        put(net.C_modules[0].bias, acc['enc_bias'].clone())               # inp = enc + C(comm): both biases see d inp
    H = net.hid_size
    put(net.f_module.weight_ih, acc['w_cat_t'][:H].t())
    put(net.f_module.weight_hh, acc['w_cat_t'][H:].t())
    put(net.f_module.bias_ih, acc['b_cat'].clone())
    put(net.f_module.bias_hh, acc['b_cat'].clone())
    off = 0
    for hd in net.heads:
        A = hd.weight.shape[0]
        put(hd.weight, acc['w_heads'][off:off + A])
        put(hd.bias, acc['b_heads'][off:off + A])
        off += A
    put(net.value_head.weight, acc['w_heads'][off:off + 1])
    put(net.value_head.bias, acc['b_heads'][off:off + 1])
