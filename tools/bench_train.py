"""Throughput of the update path Trainer.train_batch (rollout + compute_grad + RMSprop), PP-hard by default:
python tools/bench_train.py [nenvs] [updates] [native|autograd] [workload] [dense_obs 0|1] [gate_split 0|1] [collection 0|1]   (default native: no-grad
one-launch rollout + the explicit backward through time of ic3net_amd.bptt; autograd: the rollout keeps the autograd
graph, rounds 1-2; dense_obs 0: the training rollout does not assemble observation rows nothing reads).
COMM_PASSES=<P> (with SHARE_WEIGHTS=1: one C for every pass) overrides the workload's communication passes; MULTIPASS_WINDOW=0 sends
the update of such a policy through the per-step loop instead of bptt._backward_window_multipass (the line then says which ran);
MULTIPASS_COLLECTION=1 sends its collection-mode windows (argument 7 = 1) through the window path too (args.multipass_window_collection,
off by default).  WINDOW_LAUNCH=1 sets args.window_launch: the recorded rollout of an update as one launch per window (the line says how
many windows went through it: the LSTM policies' ic3_policy_window, and the ic3_commnet_window of tj_medium_commnet_mlp, pp_hard_ic and
pp_hard_iric_tanh); WINDOW_LAUNCH_COLLECTION=1 sets args.window_launch_collection beside it: the windows of collection mode (argument 7
= 1) too; WINDOW_LAUNCH_WIDE=1 sets args.window_launch_wide beside WINDOW_LAUNCH: the windows of a hid-256 policy too;
PASSES_IN_LAUNCH_WIDE=1 sets args.passes_in_launch_wide: a hid-256 policy with COMM_PASSES 2..4 runs each step as one launch (and, with
the three window switches, its windows as one launch each).  WINDOW_RECORD_PASSES=1 sets args.window_record_passes beside WINDOW_LAUNCH:
the window launch of a COMM_PASSES 2..4 policy at hid 64 / 128 records its passes and the update reads that record instead of
re-evaluating them (the line says how many windows' backwards did).  BACKWARD_WALK=1 sets args.backward_walk: the backward through time of
pp_hard_iric_tanh as one launch per window (the line says how many windows went through it).  BACKWARD_WALK_LSTM=1 sets
args.backward_walk_lstm: the same for the LSTM policies without communication — pp_hard_iric, and any recurrent workload under
COMM_MASK_ZERO=1 (args.comm_mask_zero).  ROLLOUT_ONLY=1 times the rollout half of the timed updates by itself
(Trainer.run_batch between two synchronisations) and prints its time per step.  HID=<H> overrides
the workload's hid_size (HID=256: the hid-128 workloads at the width of pp_scaled).  BATCH_WINDOWS=<k>: an update of k windows of max_steps steps (default 1; in collection mode the first starts the streams and
the others continue them)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    updates = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    mode = sys.argv[3] if len(sys.argv) > 3 else 'native'
    wl = sys.argv[4] if len(sys.argv) > 4 else 'pp_hard'
    dense = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    split = int(sys.argv[6]) if len(sys.argv) > 6 else 1      # gate product: 1 exact bf16 split products (default), 0 fp32 MFMA
    coll = int(sys.argv[7]) if len(sys.argv) > 7 else 0       # 1: collection mode (args.auto_reset): E streams of whole episodes
    over = {}
    if os.environ.get('COMM_PASSES'):
        over['comm_passes'] = int(os.environ['COMM_PASSES'])
        if os.environ.get('SHARE_WEIGHTS', '0') == '1':
            over['share_weights'] = True
    shape = dict(hid_size=int(os.environ['HID'])) if os.environ.get('HID') else {}
    if os.environ.get('COMM_MASK_ZERO', '0') == '1':
        shape['comm_mask_zero'] = True
    tr, a = bench.build_trainer(wl, E, 0, 0, 0, **dict(over, **shape))
    if over and 'MULTIPASS_WINDOW' in os.environ:            # A/B: the window backward of comm_passes > 1 policies against the loop
        a.multipass_window_backward = os.environ['MULTIPASS_WINDOW'] == '1'
    if over and 'MULTIPASS_COLLECTION' in os.environ:
        a.multipass_window_collection = os.environ['MULTIPASS_COLLECTION'] == '1'
    a.window_launch = os.environ.get('WINDOW_LAUNCH', '0') == '1'
    a.window_launch_collection = int(os.environ.get('WINDOW_LAUNCH_COLLECTION', '0'))
    a.window_launch_wide = int(os.environ.get('WINDOW_LAUNCH_WIDE', '0'))
    a.passes_in_launch_wide = int(os.environ.get('PASSES_IN_LAUNCH_WIDE', '0'))
    a.window_record_passes = int(os.environ.get('WINDOW_RECORD_PASSES', '0'))
    a.backward_walk = int(os.environ.get('BACKWARD_WALK', '0'))
    a.backward_walk_lstm = int(os.environ.get('BACKWARD_WALK_LSTM', '0'))
    a.train_dense_obs = bool(dense) and len(sys.argv) > 5     # (default since round 5: the training rollout assembles no obs rows)
    a.gate_split = bool(split)
    a.auto_reset = bool(coll)
    a.native_update = mode == 'native'
    a.bptt_two_chains = os.environ.get('TWO_CHAINS', '1') == '1'     # A/B: the backward's launches as two concurrent chains of envs
    a.fused_loss = os.environ.get('FUSED_LOSS', '1') == '1'           # A/B: compute_grad's losses + their gradients as one launch
    a.enc_window = os.environ.get('ENC_WINDOW', '1') == '1'           # A/B: the encoder backward's stage 1 once per window
    a.__dict__.update(gamma=1.0, normalize_rewards=False, entr=0, value_coeff=0.01, advantages_per_action=False,
                      batch_size=int(os.environ.get('BATCH_WINDOWS', '1')) * E * a.max_steps)
    tune = os.environ.get('TUNE', '1') == '1'
    if tune:                                  # TunableOp picks the GEMM solutions during the first (untimed) update
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_filename(os.path.join(os.environ.get('TMPDIR', '/tmp'), 'ic3_tunableop_%d.csv' % os.getpid()))
    tr.train_batch(0)
    if tune:
        torch.cuda.tunable.tuning_enable(False)
    import gc
    gc.collect()
    gc.freeze()
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    rollout_only = os.environ.get('ROLLOUT_ONLY', '0') == '1'
    if rollout_only:                                          # the rollout half of every timed update (run_batch), timed by itself
        spent, inner = [0.0], tr.run_batch

        def timed_run_batch(epoch):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = inner(epoch)
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t
            return out
        tr.run_batch = timed_run_batch
    t0 = time.perf_counter()
    steps = 0
    for u in range(updates):
        st = tr.train_batch(u)
        steps += st['num_steps']
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    knet = tr._kernel_net()
    if rollout_only:
        nsteps = updates * int(os.environ.get('BATCH_WINDOWS', '1')) * a.max_steps
        print("rollout [%s hid=%d comm_passes=%s%s passes_in_launch_wide=%d] E=%d: %.1f us per step (%d steps of %d updates; %d step launches "
              "in the process)" % (wl, a.hid_size, over.get('comm_passes', '-'), " shared" if over.get('share_weights') else "",
                                   a.passes_in_launch_wide, E, spent[0] / nsteps * 1e6, nsteps, updates, getattr(knet, 'mega_steps', 0)))
        return
    passes = "" if not over else " comm_passes=%d%s (window backwards %d, chunk of %s steps; loop backwards %d)" % (
        over['comm_passes'], " shared" if over.get('share_weights') else "", getattr(knet, 'multipass_window_backwards', 0),
        getattr(knet, 'multipass_window_chunk', '-'), getattr(knet, 'multipass_loop_backwards', 0))
    label = wl + (" hid=%d" % a.hid_size if shape else "") + passes + (" (obs rows assembled in the rollout)" if a.train_dense_obs else "") + ("" if split else " (fp32 MFMA gate product)") + \
        (" (collection mode: %d whole episodes)" % int(st['num_episodes']) if coll else "") + \
        (" (window_launch: %d windows in one launch each)" % getattr(knet, 'window_launches', 0) if a.window_launch else "") + \
        (" (passes_in_launch_wide)" if a.passes_in_launch_wide else "") + \
        (" (window_record_passes: %d windows' backwards read the launch's record)" % getattr(knet, 'multipass_recorded_windows', 0)
         if a.window_record_passes else "") + \
        (" (backward_walk: %d windows walked in one launch each)" % getattr(tr.policy_net, 'rnn_backward_walks', 0) if a.backward_walk else "") + \
        (" (backward_walk_lstm: %d windows walked in one launch each)" % getattr(tr.policy_net, 'lstm_backward_walks', 0)
         if a.backward_walk_lstm else "")
    print("train_batch [%s] %s E=%d: %.0f env-steps/s = %.2f M agent-steps/s (%.2f s per update of %d env-steps), "
          "peak mem %.1f GB, gemm %s" % (mode, label, E, steps / dt, a.nagents * steps / dt / 1e6, dt / updates,
                                         steps // updates, torch.cuda.max_memory_allocated() / 2 ** 30,
                                         'TunableOp' if tune else 'default'))


if __name__ == '__main__':
    main()
