// commnet_fwd.hip — the NON-recurrent CommNet module (comm.py:127-129, 179-205, 220-224, 228-239) after the encoder, all
// communication passes in ONE launch — ic3_commnet_forward:
//     x = tanh(enc)                    enc = encoder(obs) incl. its bias (caller: sparse gather or dense GEMM)
//     h_0 = x
//     h_{i+1} = tanh(x + f_modules[i](h_i) + C_modules[i](comm(h_i)))      i = 0 .. comm_passes - 1
//     out = [log_softmax(heads_k(h)) ... | value_head(h)]
// A workgroup owns 64 rows = whole envs (the communication block mixes the agents of one env only).  The tile [comm | h]
// lives in LDS as the A operand; pass i's [C_i | F_i] (H x 2H, packed by ic3_commnet_pack like the C weights of
// policy_step.hip) streams from L2 as the B operand of v_mfma_f32_32x32x2_f32 — exact fp32 — x and the accumulators stay
// in registers in the MFMA C/D layout, tanh on the hardware transcendental unit (|error| <= ~2e-7, bar 1e-5).
// This is f3 coverage ("other policy variants"), not the headline path: one resident workgroup per CU at
// H >= 128, no store pacing, plain loops.
//
// Round 4 — ic3_commnet_step: the WHOLE rollout iteration of trainer.py:43-108 for the non-recurrent module as one launch
// (KIND = IC3_ENV_PP / IC3_ENV_TJ instantiations of the same kernel): window descriptors of the tile's envs in LDS ->
// the dense observation rows of the state acted on (pp/tj_obs_store_run: every element evaluated and stored once) -> sparse
// encoder gather (comm.py:119) -> tanh -> the communication passes above -> heads, log_softmax -> Philox inverse-CDF draws
// (action_utils.py:32-36, the counters of ic3_env_sample_actions) -> env.step (pp/tj_step_lanes: the device functions the
// stand-alone step kernels and policy_step_kernel run).  Five launches per step before (encode, this kernel's policy part,
// draws, step, obs).
#include <type_traits>
#include <hip/hip_runtime.h>

#include "env_device.hpp"
#include "ic3_common.hpp"
#include "ps_common.hpp"
#include "step_launch.hpp"

namespace ic3 {

typedef float cn_f32x4 __attribute__((ext_vector_type(4)));
typedef float cn_f32x16 __attribute__((ext_vector_type(16)));

struct CommnetArgs {
    const float* enc;          // [R][H]
    const float* wp;           // [passes][2H/8][H][2][4] packed [C_i | F_i]
    const float* bias;         // [passes][H]  C_i.bias + f_i.bias
    const float* head_w;       // [OT][H]
    const float* head_b;       // [OT]
    const int32_t* alive_in;   // [R] or null
    const int32_t* comm_in;    // [R] or null
    float* out;                // [R][OT]
    float* h_out;              // [R][H] or null: the final hidden state (tests; the tanh recurrence: h_t)
    const float* h_in;         // [R][H] or null.  Non-null = the tanh RECURRENCE of models.RNN (models.py:68-92, rnn_type 'MLP'):
                               // h_t = tanh(affine1(obs) + affine2(h_{t-1})): x = enc WITHOUT the tanh, h_0 = h_in (one pass, comm off)
    int E, N, EPT, passes, mode_avg, comm_zero, nheads, OT, a0, a1, a2, a3;
    int n_full, EPTs;          // tiles [0, n_full) hold EPT envs, the tiles behind them EPTs envs (<= 32 rows: one 32-row MFMA tile)
    // ic3_commnet_step (KIND != 0): the env side of the iteration
    const cn_f32x4* Wt;        // encoder.weight^T [obs_dim][H/4]
    const cn_f32x4* enc_bias;  // encoder.bias [H/4]
    const cn_f32x4* loc_table; // ic3_env_encode_table or null
    float* obs;                // [E][N][obs_dim] or null: rows of the state acted on
    int32_t* action;           // [nheads][R]
    int obs_dim, G, tile_words;
    const void* wp3;           // or null: per pass three exact bf16 planes of [C_i | F_i] in fragment order (ic3_commnet_pack_split)
    int auto_reset;            // env handle in auto-reset mode: an env with t == 0 starts an episode — nobody is dead yet and
                               // the gate is 0 (trainer.py:41-46, quirks Q21 / Q22); the module carries no other state
    uint32_t seed, gid0;
    const int32_t* episode;
    const int32_t* tstep;
    StepOut so;
    PPState pp;
    TJState tj;
    // ic3_commnet_forward_record (RECORD): h_0 .. h_passes of every row, slot i at h_pass + i * h_pass_stride floats.  Behind every
    // other field: the offsets the other instantiations read their arguments at stay where they were.
    float* h_pass;             // [passes + 1][R][H]
    long long h_pass_stride;
    // WIN instantiations (ic3_policy_step on an ic3_commnet_window): T steps in one launch.  The pointers above are those of step 0
    // (h_in: slot 0 of the tanh recurrence's record); window_step_args() moves them to step t.  (Behind every other field, as above.)
    int win_T;                  // steps of the window
    int win_alive, win_comm;    // where the masks of step t >= 1 come from (IC3_WINDOW_ALIVE_* / IC3_WINDOW_COMM_*)
    int win_nfld;               // fields of the handle's state block
    const int32_t* win_state;   // the state block; field f: words [win_off[f], win_off[f] + E * win_per[f]), env-major
    int32_t* win_snaps;         // [T][win_snap_words] or null: the state entering step t, stored by the tiles that own it
    long long win_snap_words;
    float* win_h_fin;           // [T][R][H] or null: the final hidden state of every step
    int win_off[16], win_per[16];
};

// The arguments of step t of a window (WIN), as policy_step.hip's window_step_args: every per-step pointer moved by t steps, offsets
// in 64 bits; the masks of a step t >= 1 are what step t - 1 wrote.  The tanh recurrence reads slot t of its record and writes slot
// t + 1; without it h_out is the step's slot of h_fin.
template <int H>
__device__ __forceinline__ void window_step_args(CommnetArgs& a, int t)
{
    const long long R = (long long)a.E * a.N;
    const int32_t* const alive0 = a.so.alive_out;
    const int32_t* const action0 = a.action;
    if (a.win_h_fin) a.win_h_fin += t * R * H;
    if (a.h_in) {
        a.h_in += t * R * H;
        a.h_out = const_cast<float*>(a.h_in) + R * H;
    } else {
        a.h_out = a.win_h_fin;
        a.win_h_fin = nullptr;
    }
    a.out += t * R * a.OT;
    a.action += (long long)t * a.nheads * R;
    a.so.reward += t * R;
    a.so.done += (long long)t * a.E;
    if (a.so.alive_out) a.so.alive_out += t * R;
    if (a.so.comp_out) a.so.comp_out += t * R;
    if (t > 0) {
        a.alive_in = a.win_alive == IC3_WINDOW_ALIVE_PREV ? alive0 + (t - 1) * R : nullptr;
        a.comm_in = a.win_comm == IC3_WINDOW_COMM_LAST_HEAD ? action0 + ((long long)(t - 1) * a.nheads + a.nheads - 1) * R : nullptr;
    }
}

// Wave priority (policy_step.hip: the phases around a matrix product are dependent chains on the tile's critical path, the
// product is throughput work): 3 outside the [comm | h] product, 0 inside.
#define CN_PRIO(p) __builtin_amdgcn_s_setprio(p)

// NARROW (round 6): one pass with the communication block off and split products — the IC baseline's stand-in and the tanh
// recurrence — keeps only the h half of the A tile (33.8 instead of 66.5 KB at H = 128; the heads' weights in a region of their
// own): THREE workgroups per CU instead of two, so that the obs stores of one tile overlap the matrix work / dependent chains of
// two others (the kernel has no in-stream store pacing: a tile's stores and its products do not overlap inside a workgroup).
// RECORD (ic3_commnet_forward_record, KIND 0, the wide tile): the tile's h rows also go to the h_pass ring behind x and behind every
// pass — what the window backward of the module differentiates (ic3_commnet_backward); `out` may be null there (no heads).  A
// template flag: the other instantiations carry no trace of it.
// WIN (ic3_policy_step on an ic3_commnet_window): the step body inside a loop over the T steps of a window, built as
// policy_step_kernel's WIN.  The tile plan is fixed for the launch; every step reads the arguments again and moves them to its step
// (window_step_args), reads the masks step t - 1 left and its envs' counters from the state block, stores the tile's share of the env
// snapshot in front of env.step, and ends with the hand-off to the next step.  No dense obs rows in this form: the PP run-based
// store and the TJ zero fill / patches are compiled out.  WIN = 0 compiles to what it was.
template <int H, int KIND = 0, bool NARROW = false, bool RECORD = false, int WIN = 0>
__global__ __launch_bounds__(2 * H, (H <= 128) ? (NARROW ? 3 : 2) : 1) void commnet_forward_kernel(CommnetArgs a)
{
    static_assert(!RECORD || (KIND == 0 && !NARROW), "the recording instantiation is the plain forward's");
    static_assert(!WIN || (KIND != 0 && !RECORD), "the window form exists for the env instantiations");
    for (int step = 0;; ++step) {   // (one iteration unless WIN: the step of the window)
    if constexpr (WIN != 0) {                                    // WIN: the arguments again for every step (kernarg segment),
        reload_args(a);                                          // nothing of them lives across a step.  The parameter itself is
        window_step_args<H>(a, step);                            // overwritten: a local copy behind a reference changed the code of
    }                                                            // the other instantiations (profiles/r21/commnet_window_codegen.txt)
    CN_PRIO(3);
    constexpr int K = 2 * H, LDA = (NARROW ? H : K) + 4, LDA4 = LDA / 4, NT = 2 * H, H4 = H / 4, KB = K / 8, BM = 64;
    constexpr int HO = NARROW ? 0 : H, HO4 = HO / 4;             // column of the h half inside the tile
    IC3_DYNAMIC_LDS(float, smem);
    float* const As = smem;                                      // [BM][LDA]: cols [0,H) comm, [H,2H) h  (NARROW: h alone)
    cn_f32x4* const As4 = reinterpret_cast<cn_f32x4*>(smem);
    float* const sm = As + BM * LDA;                             // [BM] m_j = alive_j * comm_action_j
    float* const sscale = sm + BM;                               // [BM] per-env 1 / (n_alive - 1)
    int32_t* const sal = reinterpret_cast<int32_t*>(sscale + BM);   // [BM] alive flags
    float* const zl = reinterpret_cast<float*>(sal + BM);        // [BM][16] logits
    int32_t* const sact = reinterpret_cast<int32_t*>(zl + BM * 16);   // [BM] env action (head 0) of every row      (KIND != 0)
    uint32_t* const rmask = reinterpret_cast<uint32_t*>(sact + BM);   // [BM] window cells of a row that carry a count
    int32_t* const sep = reinterpret_cast<int32_t*>(rmask + BM); // [BM] episode counters of the tile's envs (Philox key)
    int32_t* const sts = sep + BM;                               // [BM] step counters
    int32_t* const tile = sts + BM;                              // env descriptors of the tile's envs
    int tid_v = threadIdx.x;
    if constexpr (WIN != 0) IC3_OPAQUE_VGPR(tid_v);              // (per step: nothing derived from it is hoisted out of the step loop)
    const int tid = tid_v, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int col = 32 * w + li, N = a.N;
    const int bid = blockIdx.x;
    const bool short_tile = bid >= a.n_full;                      // (plan_commnet_tiles: full tiles first, short ones behind)
    const int e0 = short_tile ? a.n_full * a.EPT + (bid - a.n_full) * a.EPTs : bid * a.EPT;
    const int nenv = min(short_tile ? a.EPTs : a.EPT, a.E - e0), rows = nenv * N;
    const bool two = rows > 32;                                  // the second 32-row MFMA tile holds rows (workgroup-uniform)
    const size_t r0 = (size_t)e0 * N;
    const int WW = (KIND == 0) ? 0 : (KIND == IC3_ENV_PP) ? (2 * a.pp.v + 1) * (2 * a.pp.v + 1) : (2 * a.tj.v + 1) * (2 * a.tj.v + 1);
    const int total = a.pp.Np + a.pp.nprey;
    const int nsegE = N * WW;
    const int tjw = tj_tile_words(N, WW);
    const float invN = 1.0f / (float)N;
    (void)total;
    (void)tjw;

    // ---- masks and per-env scale (comm.py:102-107,175-177,194-196) ---------------------------------------------------------
    if (tid < BM) {
        const bool in = tid < rows;
        int al = (in && a.alive_in) ? a.alive_in[r0 + tid] : 1;
        int cm = (in && a.comm_in) ? a.comm_in[r0 + tid] : 1;
        if constexpr (KIND != 0) {
            if (a.auto_reset && in && a.tstep[e0 + div_small(tid, invN)] == 0) {   // the env starts an episode at this step
                al = 1;
                cm = a.comm_in ? 0 : 1;                          // (a gated policy: gate 0; CommNet without a gate head talks)
                // WIN: a step t >= 1 of IC3_WINDOW_COMM_ONES stands for a per-step call that is handed a gate of ones — gated too
                if constexpr (WIN != 0) cm = (step > 0 && a.win_comm == IC3_WINDOW_COMM_ONES) ? 0 : cm;
            }
        }
        sm[tid] = in ? (float)(al * cm) : 0.f;
        sal[tid] = al;
    }
    if constexpr (KIND != 0) {
        // ---- window descriptors of the tile's envs (positions, then the per-cell table), Philox counters ----------------------
        if (tid < BM) {
            rmask[tid] = (WW <= 32) ? 0u : ~0u;
            if (tid < nenv) {
                sep[tid] = a.episode[e0 + tid];
                sts[tid] = a.tstep[e0 + tid];
            }
        }
        int2* ptab = reinterpret_cast<int2*>(tile + ((2 * a.EPT * total + 3) & ~3));
        step_desc_positions<KIND>(tile, e0, nenv, a.pp, a.tj, a.EPT, N, tid, NT);
        __syncthreads();
        const StepDescGeom dg = { N, WW, total, nsegE, tjw, invN, 1.0f / (float)max(nsegE, 1), 1.0f / (float)max(WW, 1) };
        step_desc_tab<KIND>(tile, nenv, a.pp, a.tj, a.EPT, dg, rmask, tid, NT);
        __syncthreads();
        // ---- the dense observation rows of the state this step acts on (trainer.py:49), every element stored once ------------
        // Round 6, TJ: the tile's contiguous chunk of the obs tensor (~96-98 % zeros) is ZERO-FILLED here with 16-byte stores — no
        // per-element evaluation (it was a quarter of this kernel's vector instructions, profiles/r06/pmc_commnet.txt) — and the few
        // non-zero entries are patched in behind the draws, after every wave has seen its zero stores complete (as
        // policy_step_kernel and tj_obs_fill_kernel do; bit-identical to ic3_env_observe).
        if constexpr (WIN != 0) {
            // (the window form assembles no dense rows)
        } else if constexpr (KIND == IC3_ENV_PP) {
            // (PP rows — 145 KB per env — keep the run-based store, every element evaluated and stored once: with the zero fill the
            //  wait for a tile's 872 KB of stores in front of the patches holds the workgroup's CU slot; IC launch 0.294 against 0.261 ms)
            if (a.obs) {
                const int vocab = a.pp.dim * a.pp.dim + 4;
                // the tanh recurrence streams h_in / h_out (84 MB per launch) next to the rows: with plain stores the rows wash them out of
                // the L2 (0.275 against 0.254 ms per PP-hard launch); without that traffic plain stores are the faster ones (IC: 0.245
                // against 0.259 ms) — same-box A/B, profiles/r06/commnet_ept_sweep.txt
                if ((vocab & 3) == 0 && a.h_in) pp_obs_store_run<true>(ptab, a.obs, e0, nenv, nsegE, vocab, tid, NT, 0, 1);
                else if ((vocab & 3) == 0) pp_obs_store_run<false>(ptab, a.obs, e0, nenv, nsegE, vocab, tid, NT, 0, 1);
                else pp_obs_store_run_scalar(ptab, a.obs, e0, nenv, nsegE, vocab, tid, NT, 0, 1);
            }
        } else if (a.obs) {
            const long long b0 = (long long)e0 * N * a.obs_dim;  // first float of the tile's chunk
            const long long L = (long long)nenv * N * a.obs_dim;
            float* out = a.obs + b0;
            const int head = (int)((4 - (b0 & 3)) & 3);
            const long long nb = (L - head) >> 2;
            const int tail = (int)((L - head) & 3);
            if (tid < head) out[tid] = 0.0f;
            if (tid < tail) out[head + 4 * nb + tid] = 0.0f;
            cn_f32x4* out4 = reinterpret_cast<cn_f32x4*>(out + head);
            const cn_f32x4 z4 = { 0.f, 0.f, 0.f, 0.f };
            const int o = (int)(((b0 + head) >> 2) & 63);        // 1 KiB-aligned wave stores
            long long j = tid - o;
            if (j < 0) j += NT;
            for (; j < nb; j += NT) out4[j] = z4;   // (plain stores: the rows are small — 21 KB per env — and the patches then meet their lines
                                                    //  in the L2; non-temporal: 0.146 against 0.143 ms per TJ-medium launch)
        }
        // ---- x = tanh(encoder(obs)) as a sparse gather (comm.py:119,127-129) -> h half ------------------------------------------
        const PtrRows encW = { a.Wt }, encL = { a.loc_table };
        for (int idx = tid; idx < BM * H4; idx += NT) {
            const int row = idx / H4, c4 = idx - row * H4;
            cn_f32x4 v = { 0.f, 0.f, 0.f, 0.f };
            if (row < rows) {
                const int el = div_small(row, invN), aa = row - el * N;
                if constexpr (KIND == IC3_ENV_PP) {
                    v = pp_encode_row_t(tile + el * total, tile + a.EPT * total + el * total, ptab + el * nsegE, aa, c4, H4, WW,
                                        a.pp.dim * a.pp.dim + 4, a.pp.dim, encW, a.enc_bias, encL, rmask[row]);
                } else {
                    v = tj_encode_row_t(tj_tile_at(tile + el * tjw, N), a.tj, aa, c4, H4, encW, a.enc_bias, encL, rmask[row]);
                }
                if (!a.h_in) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = fast_tanh(v[q]);
                }
            }
            As4[row * LDA4 + HO4 + c4] = v;
        }
    } else {
    // ---- x = tanh(enc) -> h half (comm.py:127-129) ---------------------------------------------------------------------------
    for (int idx = tid; idx < BM * H4; idx += NT) {
        const int row = idx / H4, c4 = idx - row * H4;
        cn_f32x4 v = { 0.f, 0.f, 0.f, 0.f };
        if (row < rows) {
            v = *reinterpret_cast<const cn_f32x4*>(a.enc + (r0 + row) * H + 4 * c4);
            if (!a.h_in) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = fast_tanh(v[q]);
            }
        }
        As4[row * LDA4 + HO4 + c4] = v;
    }
    }
    __syncthreads();
    for (int el = tid; el < nenv; el += NT) {
        int n_alive = 0;
        for (int j = 0; j < N; ++j) n_alive += sal[el * N + j];
        sscale[el] = (a.mode_avg && n_alive > 1) ? 1.0f / (float)(n_alive - 1) : 1.0f;
    }
    // RECORD: the tile's h rows -> slot `slot` of the ring (16 bytes per lane; a workgroup owns its rows: slot 0 may be `enc` itself)
    auto record = [&](int slot) __attribute__((always_inline)) {
        float* dst = a.h_pass + (size_t)slot * (size_t)a.h_pass_stride;
        for (int idx = tid; idx < rows * H4; idx += NT) {
            const int row = idx / H4, c4 = idx - row * H4;
            *reinterpret_cast<cn_f32x4*>(dst + (r0 + row) * H + 4 * c4) = As4[row * LDA4 + HO4 + c4];
        }
    };
    if constexpr (RECORD) record(0);
    float xr[2][16];                                             // x in the MFMA C/D layout, kept for every pass
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) xr[rt][reg] = As[(32 * rt + (reg & 3) + 8 * (reg >> 2) + 4 * lh) * LDA + HO + col];
    __syncthreads();
    if (a.h_in) {
        // the tanh recurrence: h_0 = the state that entered the step (zero for an env that starts an episode here: auto-reset)
        for (int idx = tid; idx < BM * H4; idx += NT) {
            const int row = idx / H4, c4 = idx - row * H4;
            cn_f32x4 v = { 0.f, 0.f, 0.f, 0.f };
            if (row < rows) {
                bool fresh = false;
                if constexpr (KIND != 0) fresh = a.auto_reset && a.tstep[e0 + div_small(row, invN)] == 0;
                if (!fresh) v = *reinterpret_cast<const cn_f32x4*>(a.h_in + (r0 + row) * H + 4 * c4);
            }
            As4[row * LDA4 + HO4 + c4] = v;
        }
        __syncthreads();
    }

    for (int pass = 0; pass < a.passes; ++pass) {
        // ---- comm_j = m_j (S_e - m_j h_j) scale_e (closed form of comm.py:181-205) -> comm half -----------------------------
        if constexpr (!NARROW) {
            const int c4 = tid % H4;
            for (int el = tid / H4; el < nenv; el += NT / H4) {
                const cn_f32x4* hp = As4 + (el * N) * LDA4 + H4 + c4;
                const float scl = sscale[el];
                cn_f32x4 S = { 0.f, 0.f, 0.f, 0.f };
                if (!a.comm_zero)
                    for (int i = 0; i < N; ++i) S = mask_fma4(sm[el * N + i], hp[i * LDA4], S);   // (one component per instruction: ic3_common.hpp)
                for (int j = 0; j < N; ++j) {
                    const float m = a.comm_zero ? 0.f : sm[el * N + j];
                    As4[(el * N + j) * LDA4 + c4] = comm_out4(m, S, hp[j * LDA4], scl);
                }
            }
            for (int idx = rows * H4 + tid; idx < BM * H4; idx += NT) {
                const int row = idx / H4, c4p = idx - row * H4;
                As4[row * LDA4 + c4p] = cn_f32x4{ 0.f, 0.f, 0.f, 0.f };
            }
        }
        __syncthreads();
        // ---- acc = [comm | h] . [C_i | F_i]^T : lane (li, lh) of wave w reads Wp[kb][32 w + li][lh] -> k = 8 kb + 4 lh + j --
        cn_f32x16 acc[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][i] = 0.0f;
        if (NARROW || a.wp3) {
            // the product as nine exact bf16 x bf16 products per fp32 product (policy_step_kernel's gate_split):
            // the weights' three planes in fragment order, Wp3[pass][plane][kb16][wave][lane] x 16 bytes, one 16-k block ahead in
            // registers; the activations split per wave from the fp32 LDS tile (ps_split_frag).  9 x 32 cycles per 16 k against
            // 8 x 64 on the fp32 instruction.
            typedef __bf16 cn_bf16x8 __attribute__((ext_vector_type(8)));
            constexpr int KB16 = K / 16, NWv = H / 32;
            const __amdgpu_buffer_rsrc_t rw = make_rsrc(reinterpret_cast<const ps_u32x4*>(a.wp3) + (size_t)pass * 3 * KB16 * NWv * 64,
                                                        (uint32_t)(3 * KB16 * NWv * 64 * 16));
            const int wu = __builtin_amdgcn_readfirstlane(w);
            auto wb = [&](int pl, int kb) __attribute__((always_inline)) {
                return __builtin_amdgcn_raw_buffer_load_b128(rw, lane * 16, ((pl * KB16 + kb) * NWv + wu) * 1024, 0);
            };
            const int kb0 = (NARROW || a.comm_zero) ? KB16 / 2 : 0;   // (comm_mask_zero / the IC stand-in: the comm half is all zeros)
            constexpr int AOFF = NARROW ? H4 : 0;                // (NARROW: the tile starts at k = H)
            // the loop in two copies, chosen once per tile: a short tile (rows <= 32, plan_commnet_tiles) runs the first 32-row MFMA
            // tile only — a branch inside the loop cost the full tiles 5 % (profiles/r06/commnet_ept_sweep.txt)
            auto product = [&](auto two_c) __attribute__((always_inline)) {
                constexpr bool TWO = decltype(two_c)::value;
                ps_u32x4 bq[3], bn[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) bq[pl] = wb(pl, kb0);
                CN_PRIO(0);
#pragma unroll 2
                for (int kb = kb0; kb < KB16; ++kb) {
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) bn[pl] = wb(pl, kb + 1);                  // (past the end: zeros, never used)
                    ps_u32x4 ap[2][3];
                    const cn_f32x4* s0 = As4 + li * LDA4 + 4 * kb + 2 * lh - AOFF;
                    const cn_f32x4* s1 = As4 + (32 + li) * LDA4 + 4 * kb + 2 * lh - AOFF;
                    ps_split_frag(s0[0], s0[1], ap[0]);
                    if constexpr (TWO) ps_split_frag(s1[0], s1[1], ap[1]);
#pragma unroll
                    for (int pb = 0; pb < 3; ++pb)
#pragma unroll
                        for (int pa = 2; pa >= 0; --pa) {                                    // (least significant term first)
                            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cn_bf16x8, ap[0][pa]),
                                                                             __builtin_bit_cast(cn_bf16x8, bq[pb]), acc[0], 0, 0, 0);
                            if constexpr (TWO)
                                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cn_bf16x8, ap[1][pa]),
                                                                                 __builtin_bit_cast(cn_bf16x8, bq[pb]), acc[1], 0, 0, 0);
                        }
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) bq[pl] = bn[pl];
                }
            };
            if (two) product(std::true_type{});
            else product(std::false_type{});
        } else if constexpr (!NARROW) {
        const cn_f32x4* wp = reinterpret_cast<const cn_f32x4*>(a.wp) + (size_t)pass * (K * H / 4) + col * 2 + lh;
        constexpr int CH = 8;
        static_assert(KB % CH == 0, "2H / 8 is a multiple of 8");
        cn_f32x4 cb[2][CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) cb[0][k] = wp[(size_t)k * H * 2];
        CN_PRIO(0);                                              // (the phases around the product run at priority 3)
#pragma unroll 1
        for (int ch = 0; ch < KB / CH; ch += 2) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int c = ch + half;
                if (c + 1 < KB / CH) {
#pragma unroll
                    for (int k = 0; k < CH; ++k) cb[(half + 1) & 1][k] = wp[(size_t)((c + 1) * CH + k) * H * 2];
                }
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int kb = c * CH + k;
                    const cn_f32x4 a0 = As4[li * LDA4 + 2 * kb + lh];
                    const cn_f32x4 a1 = As4[(32 + li) * LDA4 + 2 * kb + lh];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], cb[half][k][j], acc[0], 0, 0, 0);
                        if (two) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], cb[half][k][j], acc[1], 0, 0, 0);
                    }
                }
            }
        }
        }
        CN_PRIO(3);
        __syncthreads();                                         // every wave has read the old h
        // ---- h' = tanh(x + F h + C comm + biases) -> h half (comm.py:222-224) ------------------------------------------------
        const float b = a.bias[pass * H + col];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int lr = 32 * rt + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                As[lr * LDA + HO + col] = fast_tanh(xr[rt][reg] + acc[rt][reg] + b);
            }
        __syncthreads();
        if constexpr (RECORD) record(pass + 1);
    }
    if constexpr (RECORD) {
        if (!a.out) return;                                      // (workgroup-uniform: the window backward needs no heads)
    }

    // ---- heads + value head (comm.py:228,239): weights -> rows [0, OT) of the comm half, logits -> zl ------------------------
    cn_f32x4* const hw4 = reinterpret_cast<cn_f32x4*>(tile + a.tile_words);          // NARROW: [16][H] the heads' weights
    for (int i = tid; i < a.OT * H4; i += NT) {
        if constexpr (NARROW) hw4[i] = reinterpret_cast<const cn_f32x4*>(a.head_w)[i];
        else As4[(i / H4) * LDA4 + i % H4] = reinterpret_cast<const cn_f32x4*>(a.head_w)[i];
    }
    if (a.h_out) {
        for (int idx = tid; idx < rows * H4; idx += NT) {
            const int row = idx / H4, c4 = idx - row * H4;
            *reinterpret_cast<cn_f32x4*>(a.h_out + (r0 + row) * H + 4 * c4) = As4[row * LDA4 + HO4 + c4];
        }
    }
    if constexpr (WIN != 0) {
        if (a.win_h_fin) {                                       // (the tanh recurrence with an h_fin record: the same rows once more)
            for (int idx = tid; idx < rows * H4; idx += NT) {
                const int row = idx / H4, c4 = idx - row * H4;
                *reinterpret_cast<cn_f32x4*>(a.win_h_fin + (r0 + row) * H + 4 * c4) = As4[row * LDA4 + HO4 + c4];
            }
        }
    }
    __syncthreads();
    for (int task = tid; task < rows * a.OT; task += NT) {
        const int row = task / a.OT, o = task - row * a.OT;
        const cn_f32x4* hp = As4 + row * LDA4 + HO4;
        const cn_f32x4* wo = NARROW ? hw4 + o * H4 : As4 + o * LDA4;
        cn_f32x4 s = { 0.f, 0.f, 0.f, 0.f };
        for (int k = 0; k < H4; ++k) s += hp[k] * wo[k];
        zl[row * 16 + o] = (s[0] + s[1]) + (s[2] + s[3]) + a.head_b[o];
    }
    __syncthreads();
    const int sizes[4] = { a.a0, a.a1, a.a2, a.a3 };
    for (int task = tid; task < rows * (a.nheads + 1); task += NT) {
        const int tr = task / (a.nheads + 1), hd = task - tr * (a.nheads + 1);
        const float* z = zl + tr * 16;
        float* orow = a.out + (r0 + tr) * a.OT;
        int off = 0;
        for (int i = 0; i < hd && i < a.nheads; ++i) off += sizes[i];
        if (hd == a.nheads) {
            orow[off] = z[off];
            continue;
        }
        const int A = sizes[hd];
        const float lse = head_log_softmax(z, orow, off, A);
        if constexpr (KIND != 0) {          // the draw of this (row, head): the counters of sample_actions_env_kernel
            const int el = div_small(tr, invN), n = tr - el * N;
            const uint32_t x = philox_x24(a.seed, a.gid0 + (uint32_t)(e0 + el), DOMAIN_SAMPLE, (uint32_t)sep[el],
                                          (uint32_t)sts[el], (uint32_t)(hd * N + n));
            const int act = draw_action(x, A, [&](int o) { return z[off + o] - lse; });
            a.action[(size_t)hd * ((size_t)a.E * N) + r0 + tr] = act;
            if (hd == 0) sact[tr] = act;
        }
    }
    if constexpr (KIND != 0) {
        // ---- the non-zero entries of the tile's obs rows, on top of the zero fill issued at the start ---------------------------
        if constexpr (KIND == IC3_ENV_TJ && WIN == 0) {
            if (a.obs) {
                IC3_WAIT_VMEM();                                 // this wave's zero stores ...
                __syncthreads();                                 // ... and every other wave's have completed
                float* orow0 = a.obs + (size_t)e0 * N * a.obs_dim;
                const float inv_q = 1.0f / (float)(nsegE + N);
                for (int sg = tid; sg < nenv * (nsegE + N); sg += NT) {
                    const int el = div_small(sg, inv_q), q = sg - el * (nsegE + N);
                    tj_obs_patch(tj_tile_at(tile + el * tjw, N), a.tj, orow0 + (size_t)el * N * a.obs_dim, a.obs_dim, WW, q);
                }
            }
        }
        // ---- WIN: the integer state ENTERING this step -> the step's snapshot, the tile's envs' words of every field (what
        //      ic3_env_snapshot copies in front of a per-step call; the layout of policy_step_kernel's WIN).  env.step below is the
        //      state's only writer and sits behind the barrier.  A tile's share of a field is at most EPT * per <= 2H words (checked
        //      by the host): every load is issued before the first store.
        if constexpr (WIN != 0) {
            if (a.win_snaps) {   // (uniform)
                const int32_t* const st = a.win_state;
                int32_t* const sn = a.win_snaps + (long long)step * a.win_snap_words;
                int32_t sv[16];
#pragma unroll
                for (int f = 0; f < 16; ++f) {
                    sv[f] = 0;
                    if (f < a.win_nfld && tid < nenv * a.win_per[f]) sv[f] = st[(long long)a.win_off[f] + (long long)e0 * a.win_per[f] + tid];
                }
#pragma unroll
                for (int f = 0; f < 16; ++f)
                    if (f < a.win_nfld && tid < nenv * a.win_per[f]) sn[(long long)a.win_off[f] + (long long)e0 * a.win_per[f] + tid] = sv[f];
            }
        }
        // ---- env.step for the tile's envs with the env-action head (env_wrappers.py:76-77) -------------------------------------
        __syncthreads();
        const int lgG = __builtin_ctz(a.G);
        for (int base = 0; base < a.EPT * a.G; base += NT) {
            const int lt = base + tid;
            const int el = lt >> lgG, n = lt - (el << lgG);
            const int e = el < nenv ? e0 + el : a.E;
            if constexpr (KIND == IC3_ENV_PP) {
                pp_step_lanes(a.pp, a.so, e, n, a.E, a.G, [&]() { return sact[el * N + n]; });
            } else {
                tj_step_lanes(a.tj, a.so, e, n, a.E, a.G, [&]() { return sact[el * N + n]; });
            }
        }
    }
    if constexpr (WIN != 0) {
        if (step + 1 < a.win_T) {   // (uniform) the hand-off to the next step
            // What step t + 1 reads back — the envs' integer state and counters (env.step above), alive[t], the last head's
            // action[t], slot t + 1 of h — was stored by OTHER lanes and waves of THIS workgroup, all of it in front of this point.
            // The pairing measured for policy_step_kernel's window (profiles/r20/window_launch.txt): every wave waits for its own
            // stores, the barrier, and an agent-scope acquire invalidates the CU's vector L1 before the next step's first load.
            // No agent-scope release (it writes the XCD's dirty L2 lines back, for nobody), no atomics.
            IC3_WAIT_VMEM();
            __syncthreads();
            IC3_ACQUIRE_AGENT();
            continue;
        }
    }
    break;
    }   // step
}

// Wp[kb][col][hh][j] = W[col][8 kb + 4 hh + j], W = [C | F] (H x 2H): the layout the kernel's B fragments read
__global__ void commnet_pack_kernel(const float* __restrict__ Cw, const float* __restrict__ Fw, float* __restrict__ Wp, int H)
{
    const long long n = (long long)H * 2 * H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 3), hh = (int)((i >> 2) & 1);
        const long long rest = i >> 3;
        const int colx = (int)(rest % H), kb = (int)(rest / H);
        const int k = 8 * kb + 4 * hh + j;
        Wp[i] = k < H ? Cw[(size_t)colx * H + k] : Fw[(size_t)colx * H + (k - H)];
    }
}

// gate_split's planes for [C | F] (H x 2H): Wp3[plane][kb16][wave][lane] = 8 x bf16 { W_plane[32 wave + li][16 kb16 + 8 lh + i] },
// the three planes an exact split of every weight (ps_split3)
__global__ void commnet_pack_split_kernel(const float* __restrict__ Cw, const float* __restrict__ Fw, ps_u32x4* __restrict__ Wp, int H)
{
    const int NWv = H / 32, KB16 = 2 * H / 16;
    const long long per = (long long)KB16 * NWv * 64;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const long long rest = i >> 6;
        const int wv = (int)(rest % NWv), kb = (int)(rest / NWv);
        const int li = lane & 31, lh = lane >> 5;
        const size_t row = (size_t)32 * wv + li;
        unsigned p[3][8];
        for (int q = 0; q < 8; ++q) {
            const int k = 16 * kb + 8 * lh + q;
            ps_split3(k < H ? Cw[row * H + k] : Fw[row * H + (k - H)], p[0][q], p[1][q], p[2][q]);
        }
        for (int pl = 0; pl < 3; ++pl) {
            ps_u32x4 v;
            for (int d = 0; d < 4; ++d) v[d] = p[pl][2 * d] | (p[pl][2 * d + 1] << 16);
            Wp[(size_t)pl * per + i] = v;
        }
    }
}

}  // namespace ic3

extern "C" int ic3_commnet_pack_split(const float* C_weight, const float* f_weight, void* wp3, int H, ic3_stream stream)
{
    using namespace ic3;
    if (!C_weight || !f_weight || !wp3 || H <= 0 || (H & 31)) return fail(-22, "ic3_commnet_pack_split: hid_size a positive multiple of 32");
    hipLaunchKernelGGL(commnet_pack_split_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, C_weight, f_weight,
                       reinterpret_cast<ps_u32x4*>(wp3), H);
    IC3_HIP(hipGetLastError());
    return 0;
}

extern "C" int ic3_commnet_forward_supported(int H, int N) { return (H == 64 || H == 128 || H == 256) && N >= 1 && N <= 64; }

extern "C" int ic3_commnet_pack(const float* C_weight, const float* f_weight, float* wp, int H, ic3_stream stream)
{
    using namespace ic3;
    if (!C_weight || !f_weight || !wp || H <= 0 || (H & 7)) return fail(-22, "ic3_commnet_pack: bad arguments");
    hipLaunchKernelGGL(commnet_pack_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, C_weight, f_weight, wp, H);
    IC3_HIP(hipGetLastError());
    return 0;
}

// ic3_commnet_forward (h_pass null) and ic3_commnet_forward_record (the RECORD instantiation; `out` null: no heads, their
// arguments are not read)
static int commnet_forward(const char* fn, const float* enc, int E, int N, int H, int comm_passes, const float* wp, const void* wp3,
                           const float* bias, const float* head_w, const float* head_b, const int32_t* head_sizes, int nheads,
                           int mode_avg, int comm_zero, const int32_t* alive_in, const int32_t* comm_in, float* out, float* h_out,
                           float* h_pass, ic3_stream stream)
{
    using namespace ic3;
    const bool heads = out || !h_pass;
    if (!enc || !wp || !bias || (heads && (!head_w || !head_b || !head_sizes || !out)) || E <= 0 || comm_passes < 1)
        return fail(-22, std::string(fn) + ": bad arguments");
    if (!ic3_commnet_forward_supported(H, N))
        return fail(-38, std::string(fn) + ": needs hid_size 64/128/256 and <= 64 agents per env");
    CommnetArgs a{};
    int sz[4] = { 0, 0, 0, 0 };
    if (heads) {
        if (int rc = parse_heads(head_sizes, nheads, fn, a.OT, sz)) return rc;
    } else {
        nheads = 0;
    }
    a.h_pass = h_pass;
    a.h_pass_stride = (long long)E * N * H;
    a.enc = enc;
    a.wp = wp;
    a.wp3 = wp3;
    a.bias = bias;
    a.head_w = head_w;
    a.head_b = head_b;
    a.alive_in = alive_in;
    a.comm_in = comm_in;
    a.out = out;
    a.h_out = h_out;
    a.E = E;
    a.N = N;
    a.EPT = 64 / N;
    a.passes = comm_passes;
    a.mode_avg = mode_avg;
    a.comm_zero = comm_zero;
    a.nheads = nheads;
    a.a0 = sz[0];
    a.a1 = sz[1];
    a.a2 = sz[2];
    a.a3 = sz[3];
    const int tiles = (E + a.EPT - 1) / a.EPT;
    a.n_full = tiles;
    a.EPTs = a.EPT;
    const size_t lds = ((size_t)64 * (2 * H + 4) + 3 * 64 + 64 * 16 + 4 * 64) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    return with_hid(H, [&](auto hid) {
        constexpr int HH = decltype(hid)::value;
        if (h_pass) return launch_kernel(commnet_forward_kernel<HH, 0, false, true>, dim3(tiles), dim3(2 * HH), lds, s, a);
        return launch_kernel(commnet_forward_kernel<HH, 0>, dim3(tiles), dim3(2 * HH), lds, s, a);
    });
}

extern "C" int ic3_commnet_forward(const float* enc, int E, int N, int H, int comm_passes, const float* wp, const void* wp3,
                                   const float* bias,
                                   const float* head_w, const float* head_b, const int32_t* head_sizes, int nheads,
                                   int mode_avg, int comm_zero, const int32_t* alive_in, const int32_t* comm_in, float* out,
                                   float* h_out, ic3_stream stream)
{
    return commnet_forward("ic3_commnet_forward", enc, E, N, H, comm_passes, wp, wp3, bias, head_w, head_b, head_sizes, nheads, mode_avg,
                           comm_zero, alive_in, comm_in, out, h_out, nullptr, stream);
}

extern "C" int ic3_commnet_forward_record(const float* enc, int E, int N, int H, int comm_passes, const float* wp, const void* wp3,
                                          const float* bias, const float* head_w, const float* head_b, const int32_t* head_sizes,
                                          int nheads, int mode_avg, int comm_zero, const int32_t* alive_in, const int32_t* comm_in,
                                          float* out, float* h_out, float* h_pass, ic3_stream stream)
{
    if (!h_pass) return ic3::fail(-22, "ic3_commnet_forward_record: bad arguments");
    return commnet_forward("ic3_commnet_forward_record", enc, E, N, H, comm_passes, wp, wp3, bias, head_w, head_b, head_sizes, nheads,
                           mode_avg, comm_zero, alive_in, comm_in, out, h_out, h_pass, stream);
}

// Envs per tile of the NARROW Predator-Prey launch (the IC baseline's stand-in, the tanh recurrence).  That launch is bound by its
// obs stores (6 % of the matrix peak): a tile costs its bytes (~ its envs) plus a fixed part (descriptors, the weights' fragments,
// the dependent chain behind the product — measured ~0.15 of one env's stores), and the launch lasts as long as the CU with the most
// tiles: the dispatcher deals the workgroups round-robin, so a tile count that is no multiple of the CU count leaves some CUs one
// tile more than the others (8192 envs of 10 agents: 1366 tiles of 6 envs = 5.3 per CU against 2048 tiles of 4 envs = 8 per CU;
// 0.254-0.260 -> 0.241-0.247 ms per launch on the same box).  Half of that imbalance is charged: late tiles on emptier CUs run faster.  Results do not depend
// on the tile size (rows are independent; the draws are keyed per env).  profiles/r06/commnet_ept_sweep.txt: six env counts x
// five tile sizes against this choice.
static int plan_store_bound_ept(int E, int ept_max)
{
    const int cus = ic3::device_cus();
    int best = ept_max;
    double best_cost = 0.0;
    for (int ept = ept_max; ept >= 1 && ept >= ept_max / 3; --ept) {
        const int tiles = (E + ept - 1) / ept;
        const double per_cu = (double)tiles / cus, worst = (double)((tiles + cus - 1) / cus);
        const double cost = 0.5 * (per_cu + worst) * (ept + 0.15);
        if (ept == ept_max || cost < best_cost - 1e-9) {
            best = ept;
            best_cost = cost;
        }
    }
    return best;
}

// Tiles of the launches that are bound by their vector / matrix work (every instantiation but the narrow Predator-Prey one): a.EPT
// = 64 / N envs fill the 64-row tile, and a tile count that is no multiple of the CU count leaves some CUs a whole tile more than the
// others (8192 envs of 10 agents: 1366 tiles = 5.3 per CU; E = 7680 / 8192 / 9216 cost 0.137 / 0.152 / 0.156 ms on TJ-medium).  As
// policy_step_kernel's plan B: as many FULL tiles as give every CU the same number, the rest as SHORT tiles of 32 / N envs (one
// 32-row MFMA tile: half the matrix work and half the rows' vector work — measured 0.5 of a full tile) dispatched
// behind them; taken when at least one round of full tiles remains and the CU with the most work ends earlier.  Results do not
// depend on the plan (GPU test).  Returns the number of workgroups.
static int plan_commnet_tiles(ic3::CommnetArgs& a)
{
    const int n_all = (a.E + a.EPT - 1) / a.EPT;
    a.n_full = n_all;
    a.EPTs = a.EPT;
    const int cus = ic3::device_cus(), epts = 32 / a.N;
    if (epts < 1) return n_all;
    const int n_full = (a.E / a.EPT) / cus * cus;
    if (n_full < cus) return n_all;
    const int n_short = (a.E - n_full * a.EPT + epts - 1) / epts;
    if (n_full / cus + 0.5 * ((n_short + cus - 1) / cus) < (double)((n_all + cus - 1) / cus) - 1e-9) {
        a.n_full = n_full;
        a.EPTs = epts;
        return n_full + n_short;
    }
    return n_all;
}

static size_t commnet_step_lds(const ic3_env* env, int H, bool narrow = false)
{
    return ((size_t)64 * ((narrow ? H : 2 * H) + 4) + 3 * 64 + 64 * 16 + 4 * 64 + ic3::step_tile_words(env) + (narrow ? 16 * H : 0)) *
           sizeof(float);
}

extern "C" int ic3_commnet_step_supported(const ic3_env* env, int H)
{
    if (!env || !ic3_commnet_forward_supported(H, env->dims.N)) return 0;
    const size_t lds = commnet_step_lds(env, H);
    return lds <= 160 * 1024 ? (int)lds : 0;
}

extern "C" int ic3_commnet_step(ic3_env* env, const float* enc_wt, const float* enc_bias, const float* loc_table, int H,
                                int comm_passes, const float* wp, const void* wp3, const float* bias, const float* head_w,
                                const float* head_b, const int32_t* head_sizes, int nheads, int mode_avg, int comm_zero, const int32_t* alive_in,
                                const int32_t* comm_in, const float* h_in, float* h_out, float* out, int32_t* action, float* obs,
                                float* reward, int32_t* done, int32_t* alive, int32_t* is_completed, ic3_stream stream)
{
    using namespace ic3;
    ic3::Range range_("ic3_commnet_step");
    if (h_in && (!h_out || h_out == h_in || comm_passes != 1 || !comm_zero))
        return fail(-22, "ic3_commnet_step: the tanh recurrence (h_in) takes one pass with the communication block off and h_out != h_in");
    if (!env || !enc_wt || !enc_bias || !wp || !bias || !head_w || !head_b || !head_sizes || !out || !action || !reward || !done ||
        comm_passes < 1)
        return fail(-22, "ic3_commnet_step: bad arguments");
    if (env->resets == 0) return fail(-22, "ic3_commnet_step: reset() has not been called");
    if (nheads < 1 || nheads > 4) return fail(-22, "ic3_commnet_step: 1..4 action heads");   // (parse_heads below checks the sizes, behind the shape check)
    const int lds = ic3_commnet_step_supported(env, H);
    if (!lds)
        return fail(-38, "ic3_commnet_step: needs hid_size 64/128/256, <= 64 agents per env and an env tile that fits in LDS (use "
                         "ic3_env_encode + ic3_commnet_forward + ic3_env_sample_actions + ic3_env_step)");
    CommnetArgs a{};
    a.wp = wp;
    a.wp3 = wp3;
    a.bias = bias;
    a.head_w = head_w;
    a.head_b = head_b;
    a.alive_in = alive_in;
    a.comm_in = comm_in;
    a.out = out;
    a.h_in = h_in;
    a.h_out = h_out;
    a.passes = comm_passes;
    a.mode_avg = mode_avg;
    a.comm_zero = comm_zero;
    a.nheads = nheads;
    int sz[4];
    if (int rc = parse_heads(head_sizes, nheads, "ic3_commnet_step", a.OT, sz)) return rc;
    a.a0 = sz[0];
    a.a1 = sz[1];
    a.a2 = sz[2];
    a.a3 = sz[3];
    a.Wt = reinterpret_cast<const cn_f32x4*>(enc_wt);
    a.enc_bias = reinterpret_cast<const cn_f32x4*>(enc_bias);
    a.loc_table = reinterpret_cast<const cn_f32x4*>(loc_table);
    a.obs = obs;
    a.action = action;
    hipEvent_t ev0, ev1;   // one-shot (ic3_env_set_step_events): the dispatch itself stamps the caller's events
    fill_env_args(a, env, reward, done, alive, is_completed, true, ev0, ev1);
    const bool pp = env->kind == IC3_ENV_PP;
    env->touch_obs(obs);
    hipStream_t s = (hipStream_t)stream;
    // one pass, communication off, split products: the narrow tile (three workgroups per CU)
    const bool narrow = wp3 && comm_zero && comm_passes == 1;
    const size_t ldsn = commnet_step_lds(env, H, true);
    int tiles;
    if (narrow && pp && obs) {
        a.EPT = plan_store_bound_ept(a.E, a.EPT);
        tiles = (a.E + a.EPT - 1) / a.EPT;
        a.n_full = tiles;
        a.EPTs = a.EPT;
    } else {
        tiles = plan_commnet_tiles(a);
    }
    return with_hid(H, [&](auto hid) {
        constexpr int HH = decltype(hid)::value;
        const dim3 grid(tiles), block(2 * HH);
        if (narrow && pp) return launch_kernel_timed(commnet_forward_kernel<HH, IC3_ENV_PP, true>, grid, block, ldsn, s, ev0, ev1, a);
        if (narrow) return launch_kernel_timed(commnet_forward_kernel<HH, IC3_ENV_TJ, true>, grid, block, ldsn, s, ev0, ev1, a);
        if (pp) return launch_kernel_timed(commnet_forward_kernel<HH, IC3_ENV_PP>, grid, block, (size_t)lds, s, ev0, ev1, a);
        return launch_kernel_timed(commnet_forward_kernel<HH, IC3_ENV_TJ>, grid, block, (size_t)lds, s, ev0, ev1, a);
    });
}

// ic3_policy_step on an ic3_commnet_window (dispatched there by the descriptor's tag): T steps of ic3_commnet_step in one launch —
// the WIN instantiations.  `wide`: the descriptor is tagged IC3_COMMNET_WINDOW_WIDE — the same window at hid 256 and nothing else.
// Every refusal comes before the launch.
int ic3::commnet_step_window(ic3_env* env, const ic3_commnet_window* w, bool wide, float* h, float* c, const int32_t* alive_in,
                             const int32_t* comm_in, float* out, int32_t* action, float* obs, float* reward, int32_t* done,
                             int32_t* alive, int32_t* is_completed, ic3_stream stream)
{
    using namespace ic3;
    const std::string who = wide ? "ic3_policy_step (ic3_commnet_window, wide)" : "ic3_policy_step (ic3_commnet_window)";
    if (!env) return fail(-22, who + ": null handle");
    // the one-shots of the per-step calls have no meaning here (the descriptor names the records): disarmed, and the call refused
    const bool armed = env->h_out || env->c_out || env->gates_out || env->xh_out || env->ev_start || env->ev_stop;
    env->h_out = env->c_out = env->gates_out = env->xh_out = nullptr;
    env->ev_start = env->ev_stop = nullptr;
    if (armed)
        return fail(-22, who + ": ic3_env_set_hidden_out / ic3_env_set_record_out / ic3_env_set_step_events armed on the handle (disarmed; the "
                               "window's records are named by the descriptor)");
    const ic3_policy& p = w->policy;
    if (p.c_wp || p.lstm_wp || p.lstm_bias || p.lstm_wp3 || p.pass_index)
        return fail(-22, who + ": c_wp, lstm_wp, lstm_bias, lstm_wp3 and pass_index must be NULL / 0");
    if (!p.enc_wt || !p.enc_bias || !p.head_w || !p.head_b || !w->wp || !w->bias || !out || !action || !reward || !done || p.npasses < 1)
        return fail(-22, who + ": null argument, or npasses < 1");
    if (obs) return fail(-22, who + ": obs must be NULL (the window form assembles no dense observation rows)");
    if (c) return fail(-22, who + ": c must be NULL");
    if (w->T < 1) return fail(-22, who + ": T >= 1");
    if (w->recurrence != 0 && w->recurrence != 1) return fail(-22, who + ": recurrence is 0 or 1");
    if (w->recurrence ? (!h || p.npasses != 1 || !p.comm_zero) : h != nullptr)
        return fail(-22, who + ": the tanh recurrence takes h = the [T+1][E*N][H] record, one pass and the communication block off; "
                               "without it h must be NULL");
    if (w->snaps && w->snap_words < env->dims.state_words) return fail(-22, who + ": snap_words >= dims.state_words");
    if (w->alive_mode != IC3_WINDOW_ALIVE_ALL && w->alive_mode != IC3_WINDOW_ALIVE_PREV) return fail(-22, who + ": alive_mode");
    if (w->comm_mode != IC3_WINDOW_COMM_ALL && w->comm_mode != IC3_WINDOW_COMM_LAST_HEAD && w->comm_mode != IC3_WINDOW_COMM_ONES)
        return fail(-22, who + ": comm_mode");
    if (w->alive_mode == IC3_WINDOW_ALIVE_PREV && !alive) return fail(-22, who + ": IC3_WINDOW_ALIVE_PREV needs the alive output");
    if (env->resets == 0) return fail(-22, who + ": reset() has not been called");
    if (p.nheads < 1 || p.nheads > 4) return fail(-22, who + ": 1..4 action heads");
    const int H = p.H;
    const int lds = ic3_commnet_step_supported(env, H);
    if (wide && (H == 64 || H == 128))
        return fail(-38, who + ": IC3_COMMNET_WINDOW_WIDE is the window at hid_size 256 (hid_size 64 / 128: tag the descriptor IC3_COMMNET_WINDOW)");
    if (wide && (!lds || H != 256))
        return fail(-38, who + ": needs hid_size 256, <= 64 agents per env and an env tile that fits in LDS (hid_size 64 / 128: tag the "
                               "descriptor IC3_COMMNET_WINDOW; otherwise use one call per step)");
    if (!wide && (!lds || (H != 64 && H != 128)))
        return fail(-38, who + ": needs hid_size 64 / 128, <= 64 agents per env and an env tile that fits in LDS (use one call per step)");
    if (!w->wp3) return fail(-38, who + ": needs wp3, the split products (use one call per step)");
    CommnetArgs a{};
    a.wp = w->wp;
    a.wp3 = w->wp3;
    a.bias = w->bias;
    a.head_w = p.head_w;
    a.head_b = p.head_b;
    a.alive_in = alive_in;
    a.comm_in = comm_in;
    a.out = out;
    a.h_in = w->recurrence ? h : nullptr;
    a.win_h_fin = w->h_fin;
    a.passes = p.npasses;
    a.mode_avg = p.mode_avg;
    a.comm_zero = p.comm_zero;
    a.nheads = p.nheads;
    int sz[4];
    if (int rc = parse_heads(p.head_sizes, p.nheads, who.c_str(), a.OT, sz)) return rc;
    a.a0 = sz[0];
    a.a1 = sz[1];
    a.a2 = sz[2];
    a.a3 = sz[3];
    a.Wt = reinterpret_cast<const cn_f32x4*>(p.enc_wt);
    a.enc_bias = reinterpret_cast<const cn_f32x4*>(p.enc_bias);
    a.loc_table = reinterpret_cast<const cn_f32x4*>(p.loc_table);
    a.action = action;
    hipEvent_t ev0, ev1;
    fill_env_args(a, env, reward, done, alive, is_completed, false, ev0, ev1);
    a.win_T = w->T;
    a.win_alive = w->alive_mode;
    a.win_comm = w->comm_mode;
    a.win_state = env->state;
    a.win_snaps = w->snaps;
    a.win_snap_words = w->snap_words;
    // the handle's field table: the state is one block, a field is env-major and a tile owns its envs' words of it
    if (env->fields.size() > 16) return fail(-38, who + ": more than 16 state fields");
    for (const Field& f : env->fields) {
        const int64_t per = f.count / a.E;
        if (per * a.E != f.count || per * a.EPT > 2 * H) return fail(-38, who + ": an env tile's share of a state field does not fit");
        a.win_off[a.win_nfld] = (int)f.off;
        a.win_per[a.win_nfld] = (int)per;
        a.win_nfld += 1;
    }
    const bool pp = env->kind == IC3_ENV_PP;
    hipStream_t s = (hipStream_t)stream;
    // the tile of the per-step call: narrow for one pass with the communication block off.  No launch of this form is bound by obs
    // stores: full + short tiles (an env's trajectory is the same bits in every plan)
    const bool narrow = p.comm_zero && p.npasses == 1;
    const size_t ldsn = commnet_step_lds(env, H, true);
    const int tiles = plan_commnet_tiles(a);
    auto go = [&](auto hid) {
        constexpr int HH = decltype(hid)::value;
        const dim3 grid(tiles), block(2 * HH);
        if (narrow && pp) return launch_kernel(commnet_forward_kernel<HH, IC3_ENV_PP, true, false, 1>, grid, block, ldsn, s, a);
        if (narrow) return launch_kernel(commnet_forward_kernel<HH, IC3_ENV_TJ, true, false, 1>, grid, block, ldsn, s, a);
        if (pp) return launch_kernel(commnet_forward_kernel<HH, IC3_ENV_PP, false, false, 1>, grid, block, (size_t)lds, s, a);
        return launch_kernel(commnet_forward_kernel<HH, IC3_ENV_TJ, false, false, 1>, grid, block, (size_t)lds, s, a);
    };
    if (wide) return go(std::integral_constant<int, 256>{});
    return H == 128 ? go(std::integral_constant<int, 128>{}) : go(std::integral_constant<int, 64>{});
}
