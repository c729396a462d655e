"""ctypes binding of libic3rollout.so (include/ic3_rollout.h).  No fallback: import errors are fatal."""
import ctypes as C
import os

# torch must load first: it ships its own libamdhip64 (same soname as /opt/rocm's); loading ours first would
# bind the process to a second HIP runtime that cannot see torch's device allocations.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("IC3_ROLLOUT_LIB") or os.path.join(_HERE, "csrc", "libic3rollout.so")   # (override: A/B builds)

ABI_VERSION = 601        # IC3_VERSION of include/ic3_rollout.h this binding was written against (checked at load)
ENV_PP, ENV_TJ = 1, 2
PP_MODES = {"mixed": 0, "cooperative": 1, "competitive": 2}
TJ_DIFFICULTY = {"easy": 0, "medium": 1, "hard": 2}


class PPCfg(C.Structure):
    _fields_ = [("E", C.c_int32), ("N", C.c_int32), ("nprey", C.c_int32), ("dim", C.c_int32), ("vision", C.c_int32),
                ("mode", C.c_int32), ("stay", C.c_int32), ("moving_prey", C.c_int32), ("enemy_comm", C.c_int32),
                ("seed", C.c_uint32),
                ("env_id_offset", C.c_uint32)]


class TJCfg(C.Structure):
    _fields_ = [("E", C.c_int32), ("N", C.c_int32), ("dim", C.c_int32), ("vision", C.c_int32),
                ("difficulty", C.c_int32), ("vocab_type", C.c_int32), ("add_rate_min", C.c_double),
                ("add_rate_max", C.c_double), ("curr_start", C.c_double), ("curr_end", C.c_double),
                ("seed", C.c_uint32), ("env_id_offset", C.c_uint32)]


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "E", "N", "obs_dim", "vocab", "naction", "window", "npath",
                                         "narrival", "max_route_len", "grid_h", "grid_w", "state_words")]


class Stats(C.Structure):
    _fields_ = [("success_sum", C.c_double), ("add_rate", C.c_double), ("episodes", C.c_int64),
                ("live_env_steps", C.c_int64), ("auto_success_sum", C.c_double), ("auto_episodes", C.c_int64),
                ("auto_env_steps", C.c_int64)]


class _SizedStruct(C.Structure):
    """A struct of include/ic3_rollout.h whose first field is its own size: filled at construction (the library refuses a
    struct whose struct_size is not the size it was compiled with)."""

    def __init__(self, *a, **kw):             # positional arguments start at the field behind struct_size
        super().__init__(*((0,) + a if a else a), **kw)
        self.struct_size = C.sizeof(self)


class Policy(_SizedStruct):
    """ic3_policy (include/ic3_rollout.h): host struct of device pointers for ic3_policy_step."""
    _fields_ = [("struct_size", C.c_uint32), ("H", C.c_int32), ("nheads", C.c_int32), ("head_sizes", C.c_int32 * 4), ("mode_avg", C.c_int32),
                ("comm_zero", C.c_int32), ("enc_wt", C.c_void_p), ("enc_bias", C.c_void_p), ("loc_table", C.c_void_p),
                ("c_wp", C.c_void_p), ("lstm_wp", C.c_void_p), ("lstm_bias", C.c_void_p), ("head_w", C.c_void_p),
                ("head_b", C.c_void_p), ("pass_index", C.c_int32), ("inner_pass", C.c_int32), ("gate_split", C.c_int32),
                ("npasses", C.c_int32), ("lstm_wp3", C.c_void_p), ("c_wp_pass", C.c_void_p * 4), ("enc_bias_pass", C.c_void_p * 4)]


class PolicyRecord(_SizedStruct):
    """ic3_policy_record (include/ic3_rollout.h): an ic3_policy followed by the operands of the recording inner pass; handed to
    ic3_policy_forward in place of a Policy, with inner_pass = RECORD_PASS (the tag that selects this form) and its own struct_size."""
    RECORD_PASS = 2                            # IC3_POLICY_RECORD_PASS
    _fields_ = Policy._fields_ + [("enc_add", C.c_void_p), ("h_out", C.c_void_p), ("c_out", C.c_void_p), ("gates", C.c_void_p),
                                  ("inp", C.c_void_p)]


class PolicyWindow(_SizedStruct):
    """ic3_policy_window (include/ic3_rollout.h): an ic3_policy followed by the operands of a window of T lock-steps; handed to
    ic3_policy_step in place of a Policy, with inner_pass = WINDOW (the tag that selects this form) and its own struct_size.
    WINDOW_PASSES: the same struct for npasses = 2..4 communication passes per step (no gate record).  WINDOW_WIDE: the same struct
    for the one-pass window at hid 256 (inp rows of width H).  WINDOW_WIDE_PASSES: the same struct for npasses = 2..4 at hid 256."""
    WINDOW = 3                                 # IC3_POLICY_WINDOW
    WINDOW_PASSES = 5                          # IC3_POLICY_WINDOW_PASSES
    WINDOW_WIDE = 6                            # IC3_POLICY_WINDOW_WIDE
    WINDOW_WIDE_PASSES = 8                     # IC3_POLICY_WINDOW_WIDE_PASSES
    ALIVE_ALL, ALIVE_PREV = 0, 1               # IC3_WINDOW_ALIVE_*: the alive mask of step t >= 1
    COMM_ALL, COMM_LAST_HEAD, COMM_ONES = 0, 1, 2   # IC3_WINDOW_COMM_*: the gate of step t >= 1
    _fields_ = Policy._fields_ + [("T", C.c_int32), ("alive_mode", C.c_int32), ("comm_mode", C.c_int32), ("reserved", C.c_int32),
                                  ("gates", C.c_void_p), ("inp", C.c_void_p), ("snaps", C.c_void_p), ("snap_words", C.c_int64)]


class PolicyWindowRecord(_SizedStruct):
    """ic3_policy_window_record (include/ic3_rollout.h): an ic3_policy_window followed by the passes' record arrays; handed to
    ic3_policy_step in place of a Policy, with inner_pass = WINDOW_PASSES_RECORD and its own struct_size — the npasses window at
    hid 64 / 128 that also stores every pass's activated gates, inp rows and entering (h, c)."""
    WINDOW_PASSES_RECORD = 9                   # IC3_POLICY_WINDOW_PASSES_RECORD
    _fields_ = PolicyWindow._fields_ + [("gates_pass", C.c_void_p * 4), ("inp_pass", C.c_void_p * 4), ("h_pass", C.c_void_p * 4),
                                        ("c_pass", C.c_void_p * 4)]


class CommnetWindow(_SizedStruct):
    """ic3_commnet_window (include/ic3_rollout.h): an ic3_policy header followed by the operands of a window of T ic3_commnet_step
    calls; handed to ic3_policy_step in place of a Policy, with inner_pass = WINDOW (the tag that selects this form) and its own
    struct_size.  The masks' modes are PolicyWindow's.  WINDOW_WIDE: the same struct for the window at hid 256."""
    WINDOW = 4                                 # IC3_COMMNET_WINDOW
    WINDOW_WIDE = 7                            # IC3_COMMNET_WINDOW_WIDE
    _fields_ = Policy._fields_ + [("T", C.c_int32), ("alive_mode", C.c_int32), ("comm_mode", C.c_int32), ("recurrence", C.c_int32),
                                  ("wp", C.c_void_p), ("wp3", C.c_void_p), ("bias", C.c_void_p), ("h_fin", C.c_void_p),
                                  ("snaps", C.c_void_p), ("snap_words", C.c_int64)]


class Episode(_SizedStruct):
    """ic3_episode (include/ic3_rollout.h): episode buffers in, masks and reduced statistics out."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("E", C.c_int32), ("N", C.c_int32), ("auto_reset", C.c_int32),
                ("forced_last", C.c_int32), ("gate_ones", C.c_int32), ("done", C.c_void_p), ("alive", C.c_void_p),
                ("is_completed", C.c_void_p), ("reward", C.c_void_p), ("gate", C.c_void_p), ("gate_stride", C.c_int64),
                ("live", C.c_void_p), ("alive_mask", C.c_void_p), ("episode_mask", C.c_void_p),
                ("episode_mini_mask", C.c_void_p), ("live_after", C.c_void_p), ("stats", C.c_void_p),
                ("scratch", C.c_void_p), ("counter", C.c_void_p)]


class Bptt(_SizedStruct):
    """ic3_bptt (include/ic3_rollout.h): one window of the recorded-gates backward through time."""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in ("T", "E", "N", "H", "OT", "mode_avg", "comm_zero",
                                                                        "detach_gap", "enc_first")] + \
               [("gates", C.c_void_p), ("hs", C.c_void_p), ("cs", C.c_void_p), ("dhead", C.c_void_p), ("snaps", C.c_void_p),
                ("snap_words", C.c_int64), ("alive", C.POINTER(C.c_void_p)), ("gate", C.POINTER(C.c_void_p)),
                ("row_live", C.c_void_p), ("row_keep", C.c_void_p), ("lstm_wp3_bwd", C.c_void_p), ("w_heads", C.c_void_p),
                ("c_weight", C.c_void_p), ("dh", C.c_void_p), ("dc", C.c_void_p), ("dxh", C.c_void_p),
                ("dbias_partials", C.c_void_p), ("dcw_partials", C.c_void_p), ("enc_work", C.c_void_p),
                ("dxh_step", C.c_int64), ("two_chains", C.c_int32), ("gate_events", C.POINTER(C.c_void_p))]


class BpttPasses(_SizedStruct):
    """ic3_bptt_passes (include/ic3_rollout.h): one window (or chunk of one) of the comm_passes > 1 backward through time; handed to
    ic3_bptt_backward in place of a Bptt (magic selects this form)."""
    MAGIC = 0x53534150                         # IC3_BPTT_PASSES_MAGIC: the word that selects this form (an ic3_bptt holds T there)
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32)] + \
               [(n, C.c_int32) for n in ("T", "E", "N", "H", "OT", "passes", "mode_avg", "comm_zero", "detach_gap", "enc_first",
                                         "t_first")] + \
               [("gates", C.POINTER(C.c_void_p)), ("hs", C.POINTER(C.c_void_p)), ("cs", C.POINTER(C.c_void_p)), ("dhead", C.c_void_p),
                ("snaps", C.c_void_p), ("snap_words", C.c_int64), ("alive", C.POINTER(C.c_void_p)), ("gate", C.POINTER(C.c_void_p)),
                ("lstm_wp3_bwd", C.c_void_p), ("w_heads", C.c_void_p), ("c_weight", C.POINTER(C.c_void_p)), ("dh", C.c_void_p),
                ("dc", C.c_void_p), ("dxh", C.POINTER(C.c_void_p)), ("dxh_step", C.c_int64), ("dbias_partials", C.POINTER(C.c_void_p)),
                ("dcw_partials", C.POINTER(C.c_void_p)), ("enc_work", C.c_void_p), ("row_keep", C.c_void_p),
                ("keep_before", C.c_void_p)]

    def __init__(self, *a, **kw):             # positional arguments start at T
        super().__init__(*((self.MAGIC,) + a if a else a), **kw)
        self.magic = self.MAGIC


class BpttWalk(_SizedStruct):
    """ic3_bptt_walk (include/ic3_rollout.h): a comm_zero window of a Bptt with its T steps walked in ONE launch; handed to
    ic3_bptt_backward in place of a Bptt (magic selects this form).  max_workgroups: 0 = the library's plan, > 0 caps the grid."""
    MAGIC = 0x4b4c574c                         # IC3_BPTT_WALK_MAGIC: the word that selects this form (an ic3_bptt holds T there)
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32)] + \
               [(n, C.c_int32) for n in ("T", "E", "N", "H", "OT", "detach_gap", "enc_first", "max_workgroups")] + \
               [("gates", C.c_void_p), ("hs", C.c_void_p), ("cs", C.c_void_p), ("dhead", C.c_void_p), ("snaps", C.c_void_p),
                ("snap_words", C.c_int64), ("row_live", C.c_void_p), ("row_keep", C.c_void_p), ("lstm_wp3_bwd", C.c_void_p),
                ("w_heads", C.c_void_p), ("dh", C.c_void_p), ("dc", C.c_void_p), ("dxh", C.c_void_p), ("dxh_step", C.c_int64),
                ("dbias_partials", C.c_void_p), ("enc_work", C.c_void_p)]

    def __init__(self, *a, **kw):             # positional arguments start at T
        super().__init__(*((self.MAGIC,) + a if a else a), **kw)
        self.magic = self.MAGIC


class RnnBptt(_SizedStruct):
    """ic3_rnn_bptt (include/ic3_rollout.h): one window of the tanh-recurrence baseline's backward through time."""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in ("T", "E", "N", "H", "OT", "detach_gap", "enc_first",
                                                                        "enc_window")] + \
               [("hs", C.c_void_p), ("h_last", C.c_void_p), ("dhead", C.c_void_p), ("snaps", C.c_void_p), ("snap_words", C.c_int64),
                ("a2", C.c_void_p), ("w_heads", C.c_void_p), ("row_live", C.c_void_p), ("row_keep", C.c_void_p), ("dh", C.c_void_p),
                ("dz", C.c_void_p), ("dbias_partials", C.c_void_p), ("enc_work", C.c_void_p), ("a2_grad", C.c_void_p),
                ("wgrad_scratch", C.c_void_p)]


class RnnBpttWalk(_SizedStruct):
    """ic3_rnn_bptt_walk (include/ic3_rollout.h): an RnnBptt's window with its T steps walked in ONE launch; handed to
    ic3_rnn_backward_wide in place of an RnnBptt (magic selects this form).  dbias_partials: one row per 64-row tile."""
    MAGIC = 0x4b4c4157                         # IC3_RNN_BPTT_WALK_MAGIC: the word that selects this form (an ic3_rnn_bptt holds T there)
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32)] + RnnBptt._fields_[1:] + [("reserved", C.c_int64)]

    def __init__(self, *a, **kw):             # positional arguments start at T
        super().__init__(*((self.MAGIC,) + a if a else a), **kw)
        self.magic = self.MAGIC


class MlpBptt(_SizedStruct):
    """ic3_mlp_bptt (include/ic3_rollout.h): one window of the IC baseline's (models.MLP) backward."""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in ("T", "E", "N", "H", "OT", "enc_first", "enc_window")] + \
               [("h", C.c_void_p), ("dhead", C.c_void_p), ("snaps", C.c_void_p), ("snap_words", C.c_int64), ("enc_wt", C.c_void_p),
                ("enc_bias", C.c_void_p), ("loc_table", C.c_void_p), ("a2", C.c_void_p), ("w_heads", C.c_void_p), ("x1", C.c_void_p),
                ("dz", C.c_void_p), ("de", C.c_void_p), ("dbias_partials", C.c_void_p), ("enc_work", C.c_void_p),
                ("a2_grad", C.c_void_p), ("wgrad_scratch", C.c_void_p)]


class CommnetBptt(_SizedStruct):
    """ic3_commnet_bptt (include/ic3_rollout.h): one window of the non-recurrent CommNet module's backward."""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in ("T", "E", "N", "H", "OT", "passes", "mode_avg", "comm_zero",
                                                                        "enc_first", "enc_window", "max_chunk_steps")] + \
               [("dhead", C.c_void_p), ("snaps", C.c_void_p), ("snap_words", C.c_int64), ("alive", C.c_void_p), ("gate", C.c_void_p),
                ("enc_wt", C.c_void_p), ("enc_bias", C.c_void_p), ("loc_table", C.c_void_p), ("wp", C.c_void_p), ("wp3", C.c_void_p),
                ("bias", C.c_void_p), ("w_heads", C.c_void_p), ("f_weight", C.POINTER(C.c_void_p)), ("c_weight", C.POINTER(C.c_void_p)),
                ("f_grad", C.POINTER(C.c_void_p)), ("c_grad", C.POINTER(C.c_void_p)), ("bias_grad", C.POINTER(C.c_void_p)),
                ("heads_w_grad", C.c_void_p), ("heads_b_grad", C.c_void_p), ("h_pass", C.c_void_p), ("dxh", C.c_void_p),
                ("dz", C.c_void_p), ("dx", C.c_void_p), ("de", C.c_void_p), ("dh", C.c_void_p), ("scratch", C.c_void_p),
                ("enc_work", C.c_void_p)]


EXPORTS = {
    # name: (restype, argtypes)
    "ic3_version": (C.c_int, []),
    "ic3_abi_check": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t]),
    "ic3_last_error": (C.c_char_p, []),
    "ic3_pp_create": (C.c_int, [C.POINTER(PPCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "ic3_tj_create": (C.c_int, [C.POINTER(TJCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "ic3_env_destroy": (C.c_int, [C.c_void_p]),
    "ic3_env_dims": (C.c_int, [C.c_void_p, C.POINTER(Dims)]),
    "ic3_env_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ic3_env_reset_to": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "ic3_env_step": (C.c_int, [C.c_void_p] * 7 + [C.c_void_p]),
    "ic3_env_set_auto_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_env_observe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_env_observe_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_env_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p]),
    "ic3_env_encode_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ic3_env_set_incremental_obs": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_env_encode_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p]),
    "ic3_env_snapshot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_env_encode_backward_work": (C.c_int64, [C.c_void_p, C.c_int]),
    "ic3_env_encode_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "ic3_env_encode_backward_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                     C.c_void_p]),
    "ic3_env_encode_backward_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_env_encode_backward_window_work": (C.c_int64, [C.c_void_p, C.c_int]),
    "ic3_env_encode_backward_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                                 C.c_void_p, C.c_int, C.c_void_p]),
    "ic3_env_encode_backward_window_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_env_encode_backward_window_finish_scratch": (C.c_int64, [C.c_void_p, C.c_int]),
    "ic3_env_encode_backward_window_finish_ordered": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "ic3_env_check": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ic3_env_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ic3_env_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ic3_env_state_field": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ic3_tj_get_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "ic3_tj_build_tables": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(Dims), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t]),
    "ic3_tj_get_add_rate": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ic3_env_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats), C.c_void_p]),
    "ic3_comm_masked_mean": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]),
    "ic3_comm_masked_mean_add": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
                                 + [C.c_int] * 5 + [C.c_void_p]),
    "ic3_lstm_cell": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ic3_lstm_cell_backward": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p]),
    "ic3_policy_pack_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ic3_policy_pack_split_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ic3_lstm_gates_backward_given": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ic3_comm_backward_partials": (C.c_int, [C.c_int, C.c_int]),
    "ic3_comm_backward": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 6 + [C.c_void_p]),
    "ic3_lstm_weight_grad_scratch_floats": (C.c_size_t, [C.c_longlong, C.c_int]),
    "ic3_lstm_weight_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ic3_lstm_weight_grad_wide_scratch_floats": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "ic3_lstm_weight_grad_wide": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ic3_bptt_first_chain_envs": (C.c_int, [C.c_int, C.c_int]),
    "ic3_bptt_backward_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_bptt_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_rnn_backward_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_rnn_backward_partials": (C.c_int, [C.c_longlong, C.c_int]),
    "ic3_rnn_tanh_backward_step": (C.c_int, [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_longlong, C.c_int, C.c_void_p]),
    "ic3_rnn_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_rnn_weight_grad_scratch_floats": (C.c_size_t, [C.c_longlong, C.c_int]),
    "ic3_rnn_weight_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "ic3_rnn_backward_wide_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_rnn_backward_wide_partials": (C.c_int, [C.c_longlong, C.c_int]),
    "ic3_rnn_tanh_backward_step_wide": (C.c_int, [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5 +
                                        [C.c_int, C.c_longlong, C.c_int, C.c_void_p]),
    "ic3_rnn_backward_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_rnn_weight_grad_wide_scratch_floats": (C.c_size_t, [C.c_longlong, C.c_int]),
    "ic3_rnn_weight_grad_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    "ic3_mlp_backward_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_mlp_backward_partials": (C.c_int, [C.c_longlong, C.c_int]),
    "ic3_mlp_backward_step": (C.c_int, [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_longlong, C.c_int, C.c_void_p]),
    "ic3_mlp_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_mlp_backward_wide_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_mlp_backward_wide_partials": (C.c_int, [C.c_longlong, C.c_int]),
    "ic3_mlp_backward_step_wide": (C.c_int, [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_longlong, C.c_int, C.c_void_p]),
    "ic3_mlp_backward_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_env_set_record_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_lstm_gates_backward_dx": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 11 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ic3_commnet_forward_supported": (C.c_int, [C.c_int, C.c_int]),
    "ic3_commnet_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ic3_commnet_pack_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ic3_commnet_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 +
                            [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5),
    "ic3_commnet_forward_record": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 +
                                   [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "ic3_commnet_backward_supported": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ic3_commnet_backward_chunk_steps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "ic3_commnet_backward_scratch_floats": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "ic3_commnet_pass_backward_partials": (C.c_int, [C.c_longlong, C.c_int]),
    "ic3_commnet_pass_backward": (C.c_int, [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int,
                                                                                             C.c_longlong, C.c_int, C.c_void_p]),
    "ic3_commnet_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_commnet_step_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_commnet_step": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int] +
                         [C.c_void_p] * 12),
    "ic3_lstm_gates_backward_supported": (C.c_int, [C.c_int]),
    "ic3_lstm_gates_backward": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ic3_heads_grad_scratch_floats": (C.c_size_t, [C.c_int]),
    "ic3_heads_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "ic3_env_set_hidden_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_lstm_cell_heads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_policy_heads": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                   C.c_int, C.c_void_p]),
    "ic3_sample_actions": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ic3_env_sample_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "ic3_policy_pack": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "ic3_gate_product_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ic3_policy_step_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "ic3_policy_forward": (C.c_int, [C.POINTER(Policy), C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "ic3_policy_step": (C.c_int, [C.c_void_p, C.POINTER(Policy)] + [C.c_void_p] * 12),
    "ic3_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "ic3_event_destroy": (C.c_int, [C.c_void_p]),
    "ic3_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "ic3_env_set_step_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ic3_episode_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ic3_episode_finalize": (C.c_int, [C.POINTER(Episode), C.c_void_p]),
    "ic3_loss_gradients_partials": (C.c_int, [C.c_longlong, C.c_longlong]),
    "ic3_loss_gradients": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ic3_returns_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p]),
    "ic3_random_actions": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                     C.c_int, C.c_void_p]),
}

_lib = None


class IC3Error(RuntimeError):
    pass


def lib():
    """Load libic3rollout.so (built by __graft_entry__.build() / `make -C ic3net_amd/csrc`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise IC3Error("%s is missing: build it with `make -C ic3net_amd/csrc` (hipcc, gfx950). "
                           "There is no CPU fallback." % SO_PATH)
        l = C.CDLL(SO_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        # the boundary checks itself: same header version, same struct layouts (a stale .so would read garbage otherwise)
        if l.ic3_version() != ABI_VERSION or l.ic3_abi_check(ABI_VERSION, C.sizeof(Policy), C.sizeof(Episode)) != 0:
            raise IC3Error("%s is version %d, this binding needs %d with sizeof(ic3_policy) = %d, sizeof(ic3_episode) = %d: %s"
                           % (SO_PATH, l.ic3_version(), ABI_VERSION, C.sizeof(Policy), C.sizeof(Episode),
                              l.ic3_last_error().decode("utf-8", "replace")))
        _lib = l
    return _lib


def check(rc, exc=IC3Error):
    if rc < 0:
        msg = lib().ic3_last_error().decode("utf-8", "replace")
        if rc == -38:
            raise NotImplementedError(msg)
        if rc == -22 and exc is IC3Error:
            raise ValueError(msg)
        raise exc(msg)
    return rc


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def int32_array(values, n=None):
    """A C array of int32 from a Python sequence (the head_sizes argument of the policy entry points); n: its length, zero-filled
    behind the values (ic3_policy.head_sizes)."""
    return (C.c_int32 * (len(values) if n is None else n))(*[int(a) for a in values])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
