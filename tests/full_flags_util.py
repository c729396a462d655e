"""Helpers of tests/test_full_flags_update_gpu.py.

flagged_update(case)        one train_batch of the case's policy with EVERY one-launch switch on (full_flags_cases.FULL_FLAGS): the
                            batch it rolled out, its statistics, every parameter gradient and the path counters.
replay(case, tape, dtype)   the same update as plain torch autograd in `dtype`: a second trainer from the same seed and env offset
                            (the same weights, the same env streams), every engine flag off, no fused or one-launch policy path, no
                            sparse encoder, the policy converted to `dtype`, select_action replaced by the flagged batch's actions;
                            run_batch + compute_grad.  What it shares with the flagged path is the env stepping (checked bit for bit
                            by the test) and trainer.py's mask / loss formulas; the policy forward is the modules' generic torch
                            forward, the communication block's masked mean and the return scan are the tensor programs below — no
                            HIP kernel of the project touches a float of it.  dtype = torch.float64 is the truth, torch.float32 the
                            measuring stick: torch's own fp32 error against float64 on that tape.
compare(...)                the figures: per quantity (flagged error, fp32 replay's error e_ref, bar).

Collection mode (auto_reset): the trainer's autograd rollout has no per-env episode starts (they live inside the one-launch step),
so the replay adds them around Trainer._step_body: the env handle restarts a finished env by itself in its stand-alone step too;
the wrapper gives such an env the zero state and gate 0 at its next slot and cuts the recurrence at the detach points of the env's
own step counter (trainer.py:56-60 per stream).  Predator-Prey only (no alive masks enter the policy)."""
import os

import torch

from full_flags_cases import COUNTERS, ENV_OFFSET, EXTRA_WORKLOADS, FULL_FLAGS, HYPER, SEED, T_STEPS, WINDOWS

GRAD_FLOOR, LOSS_FLOOR, FACTOR, CAP = 4e-6, 2e-6, 8.0, 1e-4
LOSSES = ('action_loss', 'value_loss', 'entropy')


def _copy(x):
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, dict):
        return {k: _copy(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_copy(v) for v in x]
    return x


def build(case):
    import bench
    for name, wl in EXTRA_WORKLOADS.items():
        bench.WORKLOADS.setdefault(name, wl)
    E = case['envs']
    tr, a = bench.build_trainer(case['workload'], E, SEED, ENV_OFFSET, 0, **case['overrides'])
    a.__dict__.update(HYPER, normalize_rewards=bool(case['normalize_rewards']), batch_size=WINDOWS * E * a.max_steps)
    a.auto_reset = case['mode'] == 'collection'
    assert a.max_steps == T_STEPS
    return tr, a


def _objects(tr):
    """The policy the trainer holds and what runs its kernels: a zero-padded twin, a baseline's stand-in."""
    net = tr.policy_net
    objs = [net, tr._kernel_net()]
    si = net.__dict__.get('_stand_in')
    if si is not None and si.net is not None:
        objs.append(si.net)
    return objs


def counters(tr):
    """The path counters (full_flags_cases.COUNTERS) — each counted where the code counts it: on the policy, its twin or its stand-in
    (what is mirrored to the owner would count twice in a sum: the largest)."""
    def read(name):
        return max(int(getattr(o, name, 0)) for o in _objects(tr))
    out = {k: read(k) for k in COUNTERS if k != 'per_step'}
    out['per_step'] = read('mega_steps') + read('commnet_steps')
    return out


def flagged_update(case, before=None):
    tr, a = build(case)
    a.__dict__.update(FULL_FLAGS)
    if before is not None:
        before(tr, a)
    raw = tr.env.env
    ordered, plain = raw.encode_backward_window_finish_ordered, raw.encode_backward_window_finish

    def finish(H, want_bias=True):                                 # the finish that repeats itself, where the env has one
        try:
            return ordered(H, want_bias=want_bias)
        except NotImplementedError:
            return plain(H, want_bias=want_bias)
    raw.encode_backward_window_finish = finish
    cap = {}
    inner = tr.compute_grad_native

    def spy(batch, records):
        cap['batch'] = type(batch)(*_copy(list(batch)))
        cap['windows'] = len(records)
        return inner(batch, records)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    torch.cuda.synchronize()
    net = tr.policy_net
    cap.update(native='batch' in cap, stat=stat, counters=counters(tr), refused=bool(getattr(tr, '_window_refused', False)),
               grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    return cap


def masked_mean(h, alive, comm_action, mode_avg, mask_self):
    """The communication block's input (comm.py:181-205) as a tensor program in h's dtype: agent i receives the sum over the OTHER
    agents j of m_j h_j, times m_i, with m = alive x gate, divided by (agents alive - 1) in 'avg' mode where more than one is
    alive.  mask_self False is comm_mask_zero: zeros."""
    E, N, _ = h.shape
    if not mask_self:
        return torch.zeros_like(h)
    al = torch.ones((E, N), dtype=h.dtype, device=h.device) if alive is None else alive.to(h.dtype)
    m = al if comm_action is None else al * comm_action.to(h.dtype)
    mh = m.unsqueeze(2) * h
    out = m.unsqueeze(2) * (mh.sum(1, keepdim=True) - mh)
    if mode_avg:
        n_alive = al.sum(1)
        out = out * torch.where(n_alive > 1, 1.0 / (n_alive - 1).clamp(min=1), torch.ones_like(n_alive)).view(E, 1, 1)
    return out


def returns(args, rewards, episode_masks, episode_mini_masks):
    """trainer.py:162-171 as the reference's loop, in the dtype of `rewards`."""
    T = rewards.shape[0]
    coop, ncoop = torch.empty_like(rewards), torch.empty_like(rewards)
    prev_c, prev_n = torch.zeros_like(rewards[0]), torch.zeros_like(rewards[0])
    for i in reversed(range(T)):
        coop[i] = rewards[i] + args.gamma * prev_c * episode_masks[i]
        ncoop[i] = rewards[i] + args.gamma * prev_n * episode_masks[i] * episode_mini_masks[i]
        prev_c, prev_n = coop[i], ncoop[i]
    return args.mean_ratio * coop.mean(dim=2, keepdim=True) + (1 - args.mean_ratio) * ncoop


def _stream_cuts(tr, a, gap):
    """Collection mode around Trainer._step_body (see the module's docstring)."""
    inner = tr._step_body
    age = [None]
    N = a.nagents
    lstm = bool(a.recurrent) and a.rnn_type == 'LSTM'

    def body(t, observe=True):
        a.auto_reset = False                                       # (the launch chain refuses the flag; the env handle restarts)
        try:
            inner(t, observe=observe)
        finally:
            a.auto_reset = True
        done = tr._buf['done'][t].to(torch.bool)                   # (E,) the step ended the env's episode
        if age[0] is None or (t == 0 and not tr._stream_continues()):
            age[0] = torch.zeros_like(done, dtype=torch.int64)
        cut = done | ((age[0] + 1) % gap == 0)
        age[0] = torch.where(done, torch.zeros_like(age[0]), age[0] + 1)
        if a.recurrent:
            def pass_on(x):
                shape = (-1, 1) if x.dim() == 2 else (-1, 1, 1)
                c = (cut.repeat_interleave(N) if x.dim() == 2 else cut).view(shape)
                d = (done.repeat_interleave(N) if x.dim() == 2 else done).view(shape)
                x = torch.where(c, x.detach(), x)
                return torch.where(d, torch.zeros_like(x), x)
            tr._prev_hid = tuple(pass_on(x) for x in tr._prev_hid) if lstm else pass_on(tr._prev_hid)
        if a.hard_attn and a.commnet and not a.comm_action_one:    # an env that starts an episode: gate 0 (trainer.py:45-46)
            tr._info['comm_action'] = tr._info['comm_action'] * (~done).to(torch.int32).unsqueeze(1)
    tr._step_body = body


def replay(case, tape, dtype):
    """See the module's docstring.  tape (slots, heads, E, N) int32: the flagged batch's actions.  Returns the batch as rolled out
    (float32 masks and rewards, `dtype` values and log-probs), run_batch's statistics, compute_grad's losses and the gradients
    divided by num_steps as train_batch does."""
    from ic3net_amd import bptt, main, ops
    from ic3net_amd import trainer as trmod
    tr, a = build(case)
    for name, typ, default in main._ENGINE_FLAGS:                  # every path switch off
        if name in FULL_FLAGS:
            setattr(a, name, False if typ == 'flag' else 0)
    a.__dict__.update(mega_policy=False, fused_policy=False, sparse_encoder_grad=False, rollout_grad=True)
    net = tr.policy_net.to(dtype)
    net.obs_encoder = net.obs_table = None                         # the dense encoder product: plain torch
    if hasattr(net, 'obs_env'):
        net.obs_env = None
    forward = net.forward

    def cast_forward(x, info={}):                                  # observations are the env's float32 rows
        x = [x[0].to(dtype), x[1]] if isinstance(x, (list, tuple)) else x.to(dtype)
        return forward(x, info)
    net.forward = cast_forward
    T = a.max_steps
    collection = case['mode'] == 'collection'
    if collection:
        assert a.env_name == 'predator_prey'
        _stream_cuts(tr, a, int(a.detach_gap))
        a.detach_gap = 10 ** 9                                     # (the window's own step counter cuts nothing)

    def taped(args, action_out, clock, out=None):
        out.copy_(tape[clock.episode * T + clock.t])
        return out
    saved = trmod.select_action, ops.comm_masked_mean, bptt._returns
    trmod.select_action, ops.comm_masked_mean, bptt._returns = taped, masked_mean, returns
    try:
        batch, stats = tr.run_batch(0)
        stats = dict(stats)
        tr.optimizer.zero_grad()
        cast = lambda xs: tuple(x.to(dtype) for x in xs)
        b = batch._replace(reward=cast(batch.reward), episode_mask=cast(batch.episode_mask),
                           episode_mini_mask=cast(batch.episode_mini_mask),
                           misc=tuple(dict(m, alive_mask=m['alive_mask'].to(dtype), live=m['live'].to(dtype)) for m in batch.misc))
        losses = tr.compute_grad(b)
    finally:
        trmod.select_action, ops.comm_masked_mean, bptt._returns = saved
    torch.cuda.synchronize()
    n = float(stats['num_steps'])
    grads = {k: p.grad.detach() / n for k, p in net.named_parameters() if p.grad is not None}
    params = {k: p.detach().clone() for k, p in net.named_parameters()}
    return dict(batch=batch, stats=stats, losses=losses, grads=grads, params=params)


def rollout_differences(flagged, truth):
    """Where the replay did NOT see the flagged episode: names of the fields that are not bit-equal (empty: the same episode)."""
    fb, tb = flagged['batch'], truth['batch']
    bad = []

    def same(name, xs, ys):
        if len(xs) != len(ys) or not all(x.shape == y.shape and torch.equal(x.float(), y.float()) for x, y in zip(xs, ys)):
            bad.append(name)
    same('reward', fb.reward, tb.reward)
    same('episode_mask', fb.episode_mask, tb.episode_mask)
    same('episode_mini_mask', fb.episode_mini_mask, tb.episode_mini_mask)
    same('alive_mask', [m['alive_mask'] for m in fb.misc], [m['alive_mask'] for m in tb.misc])
    same('live', [m['live'] for m in fb.misc], [m['live'] for m in tb.misc])
    for k in ('num_steps', 'num_episodes'):
        if float(flagged['stat'][k]) != float(truth['stats'][k]):
            bad.append(k)
    return bad


def forward_quantities(run):
    """value and the log-probability of every taken action, (slots, E * N) each, in float64."""
    b = run['batch']
    S = len(b.value)
    out = {'forward:value': torch.stack([v.detach().reshape(-1).double() for v in b.value])}
    for k in range(len(b.action_out[0])):
        lp = torch.stack([ao[k].detach().double() for ao in b.action_out])                 # (S, E, N, A_k)
        act = torch.stack([x[k] for x in b.action]).long().unsqueeze(3)                    # (S, E, N, 1)
        out['forward:logp_taken.%d' % k] = lp.gather(3, act).reshape(S, -1)
    return out


def _tensor_err(x, ref):
    return float((x.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-6)


def errors(run, truth, losses):
    """Every figure of one run against the truth: gradients and forward quantities as max |x - x64| / max(max |x64|, 1e-6), losses
    relative.  `losses`: the run's dict of the three."""
    out = {}
    fq, fq64 = forward_quantities(run), forward_quantities(truth)
    for k in fq64:
        out[k] = _tensor_err(fq[k], fq64[k])
    for k in LOSSES:
        out['loss:' + k] = abs(float(losses[k]) - float(truth['losses'][k])) / max(abs(float(truth['losses'][k])), 1e-6)
    for k, g64 in truth['grads'].items():
        if k in run['grads']:
            out['grad:' + k] = _tensor_err(run['grads'][k], g64)
    return out


def bar_of(name, e_ref):
    return max(FACTOR * e_ref, LOSS_FLOOR if name.startswith('loss:') else GRAD_FLOOR)


def compare(case, flagged, truth, stick):
    """[(quantity, flagged error, e_ref, bar)] for every forward quantity, loss and parameter gradient; IC3_FULL_FLAGS_ERRORS_OUT
    appends them to a file."""
    err = errors(flagged, truth, flagged['stat'])
    ref = errors(stick, truth, stick['losses'])
    rows = [(k, err.get(k, float('nan')), ref[k], bar_of(k, ref[k])) for k in ref]
    path = os.environ.get('IC3_FULL_FLAGS_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            for k, e, r, bar in rows:
                f.write("%-28s %-34s flagged %.3e   e_ref %.3e   bar %.3e\n" % (case['name'], k, e, r, bar))
    return rows
