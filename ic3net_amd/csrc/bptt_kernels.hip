// bptt_kernels.hip — update half (trainer.py:128-225 differentiating comm.py:134-244 over a recorded rollout): what the backward
// through time needs besides the LSTM cell's derivative (gates_bwd.hip), as hand-written launches — no library GEMM is left in
// the per-step chain of the recorded-gates path:
//
//   ic3_comm_backward     one launch per recorded step: the communication block + C's share of dL/dh_{t-1} and C.weight's
//                         gradient.  With M the per-env mixing matrix of comm.py:181-205 (symmetric: ic3_comm_masked_mean),
//                         comm = M h_prev, inp = enc + comm C^T:
//                             d h_prev = d h_direct + M (d inp . C) = d h_direct + (M d inp) . C
//                             d C     += d inp^T . comm             = (M d inp)^T . h_prev
//                         so ONE mix (of d inp, in LDS) feeds both products — the forward's comm is never formed again.  Replaces
//                         two masked-mean launches and two library products per step.
//   ic3_lstm_weight_grad  ONE launch per window of recorded steps: d[W_ih | W_hh]^T += [inp | h_prev]^T . dgates over all
//                         T x R rows at once (split-K over the CUs, fixed-order reduction) — replaces a library product per step.
//                         Hid 64 / 128; ic3_lstm_weight_grad_wide: the same call for 64 / 128 / 256 (what ic3net_amd calls).
//   ic3_bptt_backward     the loop over a window's steps, last to first, as ONE host call: cell derivative + input gradient
//                         (ic3_lstm_gates_backward_given, the heads' share of dL/dh folded in) -> ic3_comm_backward -> the sparse
//                         encoder's backward stage 1 — three launches per step, no host work between them.
//                         On an ic3_bptt_walk descriptor: a comm_zero window's T steps walked in ONE launch
//                         (lstm_gates_bwd_walk_kernel, gates_bwd.hip: dL/dh on chip, no communication to wait for).
//   ic3_rnn_tanh_backward_step / ic3_rnn_backward   the IC / IRIC baselines' tanh recurrence: one launch per recorded step
//                         (rnn_tanh_bwd_kernel), and the loop over a window's steps as one host call.
//                         ic3_rnn_backward_wide on an ic3_rnn_bptt_walk descriptor: the window's T steps walked in ONE launch
//                         (rnn_tanh_bwd_walk_kernel: a workgroup walks its 64-row tiles last step to first, dL/dh on chip).
//   ic3_rnn_weight_grad   ONE launch per window: dA2 += dz^T . (row_live h_prev) over all T x R rows (rnn_wgrad_kernel).
//   ic3_mlp_backward_step / ic3_mlp_backward   the IC baseline (models.MLP): a window is T x R independent rows, ONE launch over
//                         all of them (mlp_bwd_kernel), and the window as one host call.
//                         The rnn / mlp entries: hid 64 / 128; their _wide twins (ic3_rnn_backward_wide, ...): the same bodies for
//                         64 / 128 / 256 (what ic3net_amd calls).
//   ic3_commnet_pass_backward / ic3_commnet_backward   the NON-recurrent CommNet module: a window is T x R independent rows in T x E
//                         independent envs — per communication pass one launch of commnet_pass_bwd_kernel, ic3_comm_backward and
//                         ic3_rnn_weight_grad over all of them, and the window (in chunks of whole steps) as one host call; hid 64 / 128 / 256.
// and what sizes their buffers / says whether they run: ic3_comm_backward_partials, ic3_lstm_weight_grad[_wide]_scratch_floats,
// ic3_bptt_backward_supported, ic3_bptt_first_chain_envs, ic3_rnn_ / ic3_mlp_backward_partials and _supported,
// ic3_rnn_weight_grad_scratch_floats, and the _wide twins of the rnn / mlp ones.
// What these share exists once.  Device: bp_load1 / bp_load4 / bp_store4 (buffer access, the wave-uniform part in `soff`), bp_zero,
// bp_kslice (a weight-gradient workgroup's K slice), TanhTile<H> (the tile machine of the two tanh kernels).  Host: launch_kernel
// (ic3_common.hpp), tanh_partials / tanh_supported, wgrad_plan / wgrad_reduce (the K slices and their fixed-order sum), window_open
// (a window descriptor's opening checks), encoder_tail (the sparse encoder's stage 1 behind a window's steps).
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation — the library products these replace ran on
// the same instruction).  Layouts as gates_bwd.hip: accumulator register `reg` of a 32 x 32 block <-> block row
// (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), block column lane & 31.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <vector>

#include "enc_bwd.hpp"
#include "ic3_common.hpp"
#include "ps_common.hpp"

extern "C" int ic3_lstm_gates_backward_given(const float* gates, float* xh, int ldx, const float* h_prev, const void* lstm_wp3_bwd,
                                             const float* c_prev, const float* dh, const float* dc, float* dgates, float* dc_prev,
                                             float* dbias_partials, int accumulate, float* dxh, const float* row_live,
                                             const float* row_keep, const float* dhead, const float* w_heads, int OT, int R, int H,
                                             ic3_stream stream);

namespace ic3 {

typedef float bp_f32x2 __attribute__((ext_vector_type(2)));
typedef float bp_f32x4 __attribute__((ext_vector_type(4)));
typedef float bp_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t bp_rsrc(const void* base, long long bytes)
{
    const uint32_t n = bytes <= 0 ? 0u : (bytes > 0xffffffffll ? 0xffffffffu : (uint32_t)bytes);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}
__device__ __forceinline__ float bp_load1(__amdgpu_buffer_rsrc_t r, int voff, int soff = 0)   // (soff: the wave-uniform part)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ bp_f32x4 bp_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff = 0)
{
    return __builtin_bit_cast(bp_f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ void bp_store4(bp_f32x4 v, __amdgpu_buffer_rsrc_t r, int voff, int soff = 0)   // (past the range: dropped)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ps_u32x4, v), r, voff, soff, 0);
}
__device__ __forceinline__ void bp_mfma(bp_f32x16& acc, float x, float y)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc, 0, 0, 0);
}
template <int N>
__device__ __forceinline__ void bp_zero(bp_f32x16* acc)        // acc[0 .. N) = 0
{
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.0f;
}

// The K slice of a weight-gradient workgroup: rows [q0, q0 + nq) of the Q recorded ones (nq clipped to [0, rows_per_wg]: the
// slices behind the last row are empty), staged KT rows at a time.
struct KSlice {
    long long q0, nq;
    int nstages;
};
__device__ __forceinline__ KSlice bp_kslice(long long Q, int rows_per_wg, int KT)
{
    const long long q0 = (long long)blockIdx.x * rows_per_wg;
    long long nq = Q - q0;
    if (nq > rows_per_wg) nq = rows_per_wg;
    if (nq < 0) nq = 0;
    return KSlice{ q0, nq, (int)((nq + KT - 1) / KT) };
}

// ---------------------------------------------------------------------------------------------------------------------------
// ic3_comm_backward.  A workgroup walks tiles of `ept` whole envs (<= 64 agent rows, the tiling of policy_step_kernel); wave w
// owns hidden columns [32 w, 32 w + 32).  Per tile:
//   0. d inp rows -> LDS, mixed in place: m_j = g_j (S - g_j x_j) scale with g = alive * gate, S = sum_i g_i x_i (the closed
//      form of ic3_comm_masked_mean, same expression order)
//   1. d h_direct + m . C (64 x H x H; d h_direct is loaded INTO the accumulators), epilogue: dh_out = that * out_scale
//   2. dC[k][n] += sum_rows m[row][k] h_prev[row][n] — accumulators live across the workgroup's tiles, one partial per workgroup
// HBM per agent row: d inp, d h_direct, h_prev in, dh_out out = 4 H floats (2 KB at H = 128); MFMA: 2 x 2 H^2 flop per row.
// ---------------------------------------------------------------------------------------------------------------------------
struct CommBwdArgs {
    const float* dxh;        // [R][ldd]: columns [0, H) = d inp, [H, 2H) = d h_prev of the gate product
    const float* h_prev;     // [R][H]
    const int32_t* alive;    // [E][N] or null (everyone: quirk Q21)
    const int32_t* gate;     // [E][N] or null (everyone talks)
    const float* cw;         // C.weight [H][H] (out, in): d comm = d inp . cw
    const float* out_scale;  // [R] or null: dh_out rows times it (collection mode: the gradient that must not cross a cut)
    float* dh_out;           // [R][H]
    float* dcw_part;         // [gridDim.x][H][H]
    int ldd, E, N, ept, tiles, mode_avg, accumulate;
};

template <int H>
__global__ __launch_bounds__(2 * H, (H <= 128) ? 3 : 1) void comm_bwd_kernel(const CommBwdArgs a)
{
    constexpr int NT = 2 * H, H4 = H / 4, LDA = H + 4, LDA4 = LDA / 4, MB = H / 32, PER = 64 * H4 / NT;
    IC3_DYNAMIC_LDS(float, smem);
    float* const Am = smem;                                      // [64][LDA]
    bp_f32x4* const Am4 = reinterpret_cast<bp_f32x4*>(smem);
    float* const sg = smem + 64 * LDA;                           // [64] alive * gate of the tile's rows
    float* const sal = sg + 64;                                  // [64] alive
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int col = 32 * w + li;
    const int N = a.N;
    bp_f32x16 acc2[MB];
    bp_zero<MB>(acc2);
    const __amdgpu_buffer_rsrc_t rcw = bp_rsrc(a.cw, (long long)H * H * 4);

    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int e0 = tile * a.ept;
        const int ne = (a.E - e0) < a.ept ? (a.E - e0) : a.ept;
        const int rows = ne * N;
        const long long r0 = (long long)e0 * N;
        // ---- every load of the tile is requested here: d inp rows (-> LDS), d h_direct straight into phase 1's accumulators
        // (P is added on top of it), the masks, h_prev of this lane's (row pair, column) for phase 2.  Rows past the tile read 0.
        const __amdgpu_buffer_rsrc_t rdi = bp_rsrc(a.dxh + r0 * a.ldd, ((long long)(rows - 1) * a.ldd + H) * 4);
        const __amdgpu_buffer_rsrc_t rdd = bp_rsrc(a.dxh + r0 * a.ldd + H, ((long long)(rows - 1) * a.ldd + H) * 4);
        const __amdgpu_buffer_rsrc_t rhp = bp_rsrc(a.h_prev + r0 * H, (long long)rows * H * 4);
        bp_f32x4 v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = tid + i * NT, row = idx / H4, c4 = idx - row * H4;
            v[i] = bp_load4(rdi, (row * a.ldd + 4 * c4) * 4);
        }
        float mg = 0.f, mal = 0.f;
        if (tid < 64 && tid < rows) {
            mal = a.alive ? (float)a.alive[r0 + tid] : 1.0f;                                     // quirk Q21: no mask = everyone
            mg = mal * (a.gate ? (float)a.gate[r0 + tid] : 1.0f);
        }
        bp_f32x16 acc1[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                acc1[rt][reg] = bp_load1(rdd, (4 * lh * a.ldd + col) * 4, (32 * rt + (reg & 3) + 8 * (reg >> 2)) * a.ldd * 4);
#pragma unroll
        for (int i = 0; i < PER; ++i) Am4[(tid + i * NT) / H4 * LDA4 + (tid + i * NT) % H4] = v[i];
        if (tid < 64) {
            sg[tid] = mg;
            sal[tid] = mal;
        }
        float hpv[32];                                           // (behind the staging registers: in flight during phases 0 and 1)
#pragma unroll
        for (int s = 0; s < 32; ++s) hpv[s] = bp_load1(rhp, (lh * H + col) * 4, 2 * s * H * 4);
        __syncthreads();
        // ---- phase 0: the rows mixed per env, in place in LDS ------------------------------------------------------------
        for (int item = tid; item < ne * H4; item += NT) {
            const int el = item / H4, c4 = item - el * H4;
            float na = 0.f;
            for (int j = 0; j < N; ++j) na += sal[el * N + j];                                   // comm.py:102-107
            const int n_alive = (int)na;
            const float scale = (a.mode_avg && n_alive > 1) ? 1.0f / (float)(n_alive - 1) : 1.0f;   // comm.py:194-196, Q23
            bp_f32x4 S = { 0.f, 0.f, 0.f, 0.f };
            for (int i = 0; i < N; ++i) S = mask_fma4(sg[el * N + i], Am4[(el * N + i) * LDA4 + c4], S);   // (ic3_common.hpp: not packed)
            for (int j = 0; j < N; ++j) {
                const float m = sg[el * N + j];
                const bp_f32x4 x = Am4[(el * N + j) * LDA4 + c4];
                Am4[(el * N + j) * LDA4 + c4] = comm_out4(m, S, x, scale);
            }
        }
        __syncthreads();
        // ---- phase 1: d h_direct + m . C  (k = 8 kb + 4 lh + j: A fragment and B slot agree) ---------------------------------
        float wv[4], wn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = bp_load1(rcw, (4 * lh * H + col) * 4, j * H * 4);
#pragma unroll 2
        for (int kb = 0; kb < H / 8; ++kb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) wn[j] = bp_load1(rcw, (4 * lh * H + col) * 4, (8 * (kb + 1) + j) * H * 4);   // (past the end: 0)
            const bp_f32x4 a0 = Am4[li * LDA4 + 2 * kb + lh];
            const bp_f32x4 a1 = Am4[(32 + li) * LDA4 + 2 * kb + lh];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bp_mfma(acc1[0], a0[j], wv[j]);
                bp_mfma(acc1[1], a1[j], wv[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) wv[j] = wn[j];
        }
        {
            const __amdgpu_buffer_rsrc_t rout = bp_rsrc(a.dh_out + r0 * H, (long long)rows * H * 4);
            const __amdgpu_buffer_rsrc_t rsc = bp_rsrc(a.out_scale ? a.out_scale + r0 : a.dh_out, a.out_scale ? (long long)rows * 4 : 0);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int lc = 32 * rt + (reg & 3) + 8 * (reg >> 2);
                    float o = acc1[rt][reg];
                    if (a.out_scale) o *= bp_load1(rsc, 4 * lh * 4, lc * 4);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, o), rout, (4 * lh * H + col) * 4, lc * H * 4, 0);   // (past the tile: dropped)
                }
        }
        // ---- phase 2: dC[k][n] += sum_rows m[row][k] h_prev[row][n]: A = m^T from LDS, B = the h_prev registers ---------------
#pragma unroll 4
        for (int s = 0; s < 32; ++s) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) bp_mfma(acc2[mb], Am[(2 * s + lh) * LDA + 32 * mb + li], hpv[s]);
        }
        __syncthreads();                                         // every wave is done with the tile
    }
    float* dst = a.dcw_part + (size_t)blockIdx.x * H * H;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int k = 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (a.accumulate) dst[k * H + col] += acc2[mb][reg];
            else dst[k * H + col] = acc2[mb][reg];
        }
}

// comm_mask_zero (comm.py:40-41: C sees zeros — also the IRIC stand-in): dL/dh_{t-1} is the gate product's share alone
__global__ __launch_bounds__(256) void dh_copy_kernel(const float* __restrict__ dxh, int ldd, const float* __restrict__ out_scale,
                                                      float* __restrict__ dh_out, long long R, int H4)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < R * H4; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / H4;
        const int c4 = (int)(i - row * H4);
        bp_f32x4 v = *reinterpret_cast<const bp_f32x4*>(dxh + row * ldd + 4 * H4 + 4 * c4);
        if (out_scale) v *= out_scale[row];
        reinterpret_cast<bp_f32x4*>(dh_out)[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ic3_lstm_weight_grad.  dW[m][n] = sum_q X[q][m] D[q][n], X = [inp | h_prev] (2H columns), D = dgates (4H columns), q over
// the Q = T x R recorded rows.  Workgroup (ks, ny): K-slice ks of the rows, output columns [128 ny, 128 ny + 128), all 2H output
// rows; 4 waves as 2 (m) x 2 (n), a wave holds H x 64 of the result (128 accumulator registers at H = 128); two workgroups per
// CU, so that one's staging and barrier sit beside the other's matrix work (a single 8-wave workgroup per CU ran in lock-step:
// 106 instead of ... TFLOP/s).
// Both operands are row-major with q outermost — exactly what v_mfma_f32_32x32x2_f32 wants of a K-major pair: lane (i, kk)
// supplies X[q0 + kk][m(i)] and D[q0 + kk][n(i)], consecutive lanes read consecutive floats, no transposes anywhere.  One
// ds_read_b128 of X feeds the A operands of four m-blocks (block j takes element j: m = 4 i + j — a permutation of the output
// rows the epilogue undoes), one ds_read_b64 of D the B operands of two n-blocks: 6 LDS dwords per 8 MFMAs.
// Staging: KT = 16 rows per stage, global -> registers -> LDS, double-buffered, one barrier per stage.
// Bound: MFMA (2 Q 2H 4H flop on the fp32 instruction: 1.72 TFLOP for a PP-hard update); X is read once per column block
// (4 H / 128 times, from L2 when the blocks of a slice run together: they are gridDim.x apart, i.e. on one XCD), D once.
// Hid 256 (dW 512 x 1024): all 2H output rows in one workgroup would be 256 accumulator registers per wave, so the <256>
// instantiations ARE the tile of 128 — XW = 256 staged X columns, a wave holds 128 x 64, the LDS and the registers of <128> (two
// workgroups per CU) — on a grid (ks, 8, 2): blockIdx.z picks the inp half (output rows 0..255, source rows of stride ldi) or the
// h half (rows 256..511, times row_live) of [inp | h], so a workgroup stages ONE source and row_live touches the z = 1 workgroups
// only.  D is fetched and split once per z, X once per ny; the 16 workgroups of a slice are gridDim.x apart with ks a multiple of
// 8 (one XCD, one L2).  The slices are as many whole rounds of workgroups as keep one below 2 GB (lstm_wgrad_plan): the slices
// beyond the resident ones simply start later.  WIDE / HT fold away at 64 / 128: those code objects are the earlier ones,
// instruction for instruction.  Measured (profiles/r11/wgrad_h256.txt): 2.1 M rows 14.3 ms split / 15.8 ms fp32 against 24.6 ms for
// the two library products they replace; in a config-5 update's kernel trace one launch of 153.0 ms per 80-step window (21 M rows,
// 64 slices = two rounds; 144 TFLOP/s fp32-equivalent, 0.52 of the bf16 peak as issued — the <128> tile's share), the reduction
// 0.034 ms.  At most 24 KB per row (no L2 sharing at all) = 3.3 TB/s: matrix-bound either way, as at 128.
// ---------------------------------------------------------------------------------------------------------------------------
struct WGradArgs {
    const float* inp;        // [Q][ldi]: the first H floats of a row = inp
    const float* h;          // [Q][H]   h_prev
    const float* dg;         // [Q][4H]  dgates
    const float* row_live;   // [Q] or null: h rows times it
    float* part;             // [gridDim.x][2H][4H]
    long long Q;
    int ldi, rows_per_wg;    // rows per K slice (a multiple of 16)
};

template <int H>
__global__ __launch_bounds__(256, 2) void lstm_wgrad_kernel(const WGradArgs a)
{
    constexpr bool WIDE = H == 256;                              // blockIdx.z: the inp half or the h half of [inp | h]
    constexpr int HT = WIDE ? 128 : H;                           // output rows per wave
    constexpr int KT = 16, XW = 2 * HT, DW = 128, MB = HT / 32, NB = 2, NT = 256;
    constexpr int X4R = XW / 4, D4R = DW / 4;                    // float4 per staged row
    constexpr int XPT = KT * X4R / NT, DPT = KT * D4R / NT;      // float4 per thread and stage (4 / 2 at H = 128)
    static_assert(XPT >= 1 && DPT == 2 && (NT % X4R) == 0, "staging split");
    IC3_DYNAMIC_LDS(float, smem);
    constexpr int SW = KT * (XW + DW);                           // stage b: X at smem + b * SW, D behind it
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = w & 1, wn = w >> 1;
    const int ny = blockIdx.y;
    const KSlice sl = bp_kslice(a.Q, a.rows_per_wg, KT);
    const long long q0 = sl.q0, nq = sl.nq;
    const int nstages = sl.nstages;
    const __amdgpu_buffer_rsrc_t ri = bp_rsrc(a.inp + q0 * a.ldi, nq > 0 ? ((nq - 1) * a.ldi + H) * 4 : 0);
    const __amdgpu_buffer_rsrc_t rh = bp_rsrc(a.h + q0 * H, nq * H * 4);
    const __amdgpu_buffer_rsrc_t rd = bp_rsrc(a.dg + q0 * 4 * H + ny * DW, nq > 0 ? ((nq - 1) * 4 * H + DW) * 4 : 0);
    const __amdgpu_buffer_rsrc_t rl = bp_rsrc(a.row_live ? a.row_live + q0 : a.h, a.row_live ? nq * 4 : 0);
    // a thread stages the same (row-in-stage, column chunk) of every stage: X chunk i at row xrow + i * (NT / X4R)
    const int xrow = tid / X4R, xc4 = tid - xrow * X4R;
    const bool x_is_h = WIDE ? blockIdx.z != 0 : xc4 >= H / 4;
    const int xvoff = x_is_h ? (xrow * H + 4 * xc4 - (WIDE ? 0 : H)) * 4 : (xrow * a.ldi + 4 * xc4) * 4;
    const int xstep = (NT / X4R) * (x_is_h ? H : a.ldi) * 4;    // bytes between two of the thread's chunks
    const int drow = tid / D4R, dc4 = tid - drow * D4R;
    const int dvoff = (drow * 4 * H + 4 * dc4) * 4;

    bp_f32x4 xr[XPT], dr[DPT];
    auto fetch = [&](int s) {
        const int qb = s * KT;
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            if (x_is_h) {
                xr[i] = bp_load4(rh, xvoff + i * xstep, qb * H * 4);
                if (a.row_live) xr[i] *= bp_load1(rl, (xrow + i * (NT / X4R)) * 4, qb * 4);
            } else {
                xr[i] = bp_load4(ri, xvoff + i * xstep, qb * a.ldi * 4);
            }
        }
#pragma unroll
        for (int i = 0; i < DPT; ++i) dr[i] = bp_load4(rd, dvoff + i * (NT / D4R) * 4 * H * 4, qb * 4 * H * 4);
    };
    auto stash = [&](int b) {
        bp_f32x4* X4 = reinterpret_cast<bp_f32x4*>(smem + b * SW);
        bp_f32x4* D4 = reinterpret_cast<bp_f32x4*>(smem + b * SW + KT * XW);
#pragma unroll
        for (int i = 0; i < XPT; ++i) X4[tid + i * NT] = xr[i];
#pragma unroll
        for (int i = 0; i < DPT; ++i) D4[tid + i * NT] = dr[i];
    };
    bp_f32x16 acc[MB][NB];
    bp_zero<MB * NB>(&acc[0][0]);
    if (nstages > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
        if (more) fetch(s + 1);
        const float* Xs = smem + (s & 1) * SW;
        const float* Ds = Xs + KT * XW;
#pragma unroll
        for (int ks = 0; ks < KT / 2; ++ks) {
            const int kr = 2 * ks + lh;
            float av[MB];
            if constexpr (MB == 4) {
                const bp_f32x4 t4 = *reinterpret_cast<const bp_f32x4*>(Xs + kr * XW + wm * HT + 4 * li);
                av[0] = t4[0], av[1] = t4[1], av[2] = t4[2], av[3] = t4[3];
            } else {
                const bp_f32x2 t2 = *reinterpret_cast<const bp_f32x2*>(Xs + kr * XW + wm * HT + 2 * li);
                av[0] = t2[0], av[1] = t2[1];
            }
            const bp_f32x2 bv = *reinterpret_cast<const bp_f32x2*>(Ds + kr * DW + wn * 64 + 2 * li);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                bp_mfma(acc[mb][0], av[mb], bv[0]);
                bp_mfma(acc[mb][1], av[mb], bv[1]);
            }
        }
        if (more) stash((s + 1) & 1);
        __syncthreads();
    }
    // block (mb, nb), register reg, lane (li, lh): output row m = wm HT + MB i + mb with i = (reg & 3) + 8 (reg >> 2) + 4 lh
    // (hid 256: behind the XW rows of the other half), output column n = 128 ny + 64 wn + 2 li + nb
    float* dst = a.part + (size_t)blockIdx.x * 2 * H * 4 * H;
    const int m0 = WIDE ? (int)blockIdx.z * XW : 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            const int m = m0 + wm * HT + MB * i + mb;
            const int n = DW * ny + 64 * wn + 2 * li;
            *reinterpret_cast<bp_f32x2*>(dst + (size_t)m * 4 * H + n) = bp_f32x2{ acc[mb][0][reg], acc[mb][1][reg] };
        }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same product as EXACT bf16 split products (split != 0; the arithmetic of the rollout's gate product):
// every fp32 operand x = x1 + x2 + x3 (three bf16 terms, round-to-nearest-even, exact residuals), all nine cross products on
// v_mfma_f32_32x32x16_bf16 (a bf16 x bf16 product is exact in fp32), fp32 accumulation.  Here BOTH operands are activations, and
// the matrix instruction wants 8 consecutive k = rows q per lane at a fixed column — the transposed access of row-major data:
//   * a thread stages 8 consecutive rows of ONE column (8 four-byte loads, coalesced across the lanes: consecutive columns),
//     splits them in registers (ps_split_frag: 36 vector instructions per 8 values) and writes three 16-byte fragments — each
//     element of X and D is split ONCE per workgroup, not once per wave that multiplies with it;
//   * LDS holds the planes in fragment order, [plane][k half][column] x 16 bytes: a wave's A / B fragment is one conflict-free
//     ds_read_b128, 18 of them (4 + 2 fragments x 3 planes) per 72 MFMAs of a 16-row step.
// Same grid, tile (2H x 128 per workgroup, H x 64 per wave), K slices and reduction as the fp32 form above.  Issue bound: 9 x 32
// cycles per 32 x 32 x 16 block against 8 x 64 on the fp32 instruction (1.78 x), minus the split that does not hide under the MFMAs.
// ---------------------------------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(256, 2) void lstm_wgrad_split_kernel(const WGradArgs a)
{
    constexpr bool WIDE = H == 256;                              // blockIdx.z: the inp half or the h half of [inp | h]
    constexpr int HT = WIDE ? 128 : H;                           // output rows per wave
    constexpr int KT = 16, XW = 2 * HT, DW = 128, MB = HT / 32, NB = 2, NT = 256;
    constexpr int NGX = 2 * XW / NT;                             // 8-row groups of X per thread and stage (2 at H = 128, 1 at H = 64)
    constexpr int SQ = 3 * 2 * (XW + DW);                        // 16-byte fragments per stage: [plane][k half][column]
    typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
    IC3_DYNAMIC_LDS(float, smem);
    ps_u32x4* const frag = reinterpret_cast<ps_u32x4*>(smem);    // stage b at frag + b * SQ: X planes, then D planes
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = w & 1, wn = w >> 1;
    const int ny = blockIdx.y;
    const KSlice sl = bp_kslice(a.Q, a.rows_per_wg, KT);
    const long long q0 = sl.q0, nq = sl.nq;
    const int nstages = sl.nstages;
    const __amdgpu_buffer_rsrc_t ri = bp_rsrc(a.inp + q0 * a.ldi, nq > 0 ? ((nq - 1) * a.ldi + H) * 4 : 0);
    const __amdgpu_buffer_rsrc_t rh = bp_rsrc(a.h + q0 * H, nq * H * 4);
    const __amdgpu_buffer_rsrc_t rd = bp_rsrc(a.dg + q0 * 4 * H + ny * DW, nq > 0 ? ((nq - 1) * 4 * H + DW) * 4 : 0);
    const __amdgpu_buffer_rsrc_t rl = bp_rsrc(a.row_live ? a.row_live + q0 : a.h, a.row_live ? nq * 4 : 0);
    // X group g = tid + i NT: column g % XW, rows 8 (g / XW) .. + 7 of the stage; the D group: column tid % DW, k half tid / DW.
    // Lane part of every address in ONE VGPR (column + the group's k half), the stage / row part on the scalar ALU — an soffset
    // that depends on a VGPR, however uniform, costs a waterfall loop per load.  Which side of [inp | h] a wave stages is
    // wave-uniform (64 consecutive columns): a scalar branch.
    const int dcol = tid % DW, dkg = tid / DW;
    int xoff[NGX], loff[NGX];
    bool x_is_h[NGX];
#pragma unroll
    for (int i = 0; i < NGX; ++i) {
        const int g = tid + i * NT, c = g % XW, kg = g / XW;
        x_is_h[i] = WIDE ? blockIdx.z != 0 : __builtin_amdgcn_readfirstlane((int)(c >= H)) != 0;
        xoff[i] = x_is_h[i] ? ((c - (WIDE ? 0 : H)) + 8 * kg * H) * 4 : (c + 8 * kg * a.ldi) * 4;
        loff[i] = 8 * kg * 4;
    }
    const int doff = (dcol + 8 * dkg * 4 * H) * 4;
    float xv[NGX][8], dv[8];
    auto fetch = [&](int s) {
        const int qb = s * KT;
#pragma unroll
        for (int i = 0; i < NGX; ++i) {
            if (x_is_h[i]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[i][j] = bp_load1(rh, xoff[i], (qb + j) * H * 4);
                if (a.row_live) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[i][j] *= bp_load1(rl, loff[i], (qb + j) * 4);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[i][j] = bp_load1(ri, xoff[i], (qb + j) * a.ldi * 4);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) dv[j] = bp_load1(rd, doff, (qb + j) * 4 * H * 4);
    };
    auto stash = [&](int b) {
        ps_u32x4* f = frag + b * SQ;
        ps_u32x4 pl[3];
#pragma unroll
        for (int i = 0; i < NGX; ++i) {
            const int g = tid + i * NT, c = g % XW, kg = g / XW;
            ps_split_frag(ps_f32x4{ xv[i][0], xv[i][1], xv[i][2], xv[i][3] }, ps_f32x4{ xv[i][4], xv[i][5], xv[i][6], xv[i][7] }, pl);
#pragma unroll
            for (int p = 0; p < 3; ++p) f[(p * 2 + kg) * XW + c] = pl[p];
        }
        ps_split_frag(ps_f32x4{ dv[0], dv[1], dv[2], dv[3] }, ps_f32x4{ dv[4], dv[5], dv[6], dv[7] }, pl);
#pragma unroll
        for (int p = 0; p < 3; ++p) f[3 * 2 * XW + (p * 2 + dkg) * DW + dcol] = pl[p];
    };
    bp_f32x16 acc[MB][NB];
    bp_zero<MB * NB>(&acc[0][0]);
    // Pipeline: at the top of iteration s the registers hold stage s + 1 (requested a whole iteration ago) and LDS buffer s & 1
    // holds stage s.  The iteration is ONE basic block — the split + stash of stage s + 1 and the 72 products of stage s
    // (independent work: different LDS buffers; the compiler interleaves them), then the loads of stage s + 2 — so that the vector
    // work rides in the issue slots the matrix instructions leave (measured: 6.8 ms with the stash behind a branch and waterfall
    // loops around the loads, 5.8 ms like this, for 3.3 M rows at H = 128; the fp32 form takes 6.4 ms).  Everything is unconditional: stages past the slice read zeros (range check) and
    // stash them into a buffer nobody multiplies.
    fetch(0);
    stash(0);
    fetch(1);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < nstages; ++s) {
        const ps_u32x4* fx = frag + (s & 1) * SQ;
        const ps_u32x4* fd = fx + 3 * 2 * XW;
        ps_u32x4 bf[3][NB];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) bf[p][nb] = fd[(p * 2 + lh) * DW + 64 * wn + 32 * nb + li];
        stash((s + 1) & 1);                                      // (in front of the products in program order: the scheduler
                                                                 //  starts the vector work while the first fragments arrive)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            ps_u32x4 af[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) af[p] = fx[(p * 2 + lh) * XW + wm * HT + 32 * mb + li];
#pragma unroll
            for (int pb = 0; pb < 3; ++pb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int pa = 2; pa >= 0; --pa)                  // (least significant term first)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wg_bf16x8, af[pa]),
                                                                              __builtin_bit_cast(wg_bf16x8, bf[pb][nb]), acc[mb][nb], 0, 0, 0);
        }
        fetch(s + 2);
        __syncthreads();
    }
    // block (mb, nb), register reg, lane (li, lh): output row m = wm HT + 32 mb + (reg & 3) + 8 (reg >> 2) + 4 lh (hid 256: behind
    // the XW rows of the other half), column n = 128 ny + 64 wn + 32 nb + li
    float* dst = a.part + (size_t)blockIdx.x * 2 * H * 4 * H;
    const int m0 = WIDE ? (int)blockIdx.z * XW : 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int m = m0 + wm * HT + 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                dst[(size_t)m * 4 * H + DW * ny + 64 * wn + 32 * nb + li] = acc[mb][nb][reg];
            }
}

// dW += the K slices' partials, summed in slice order (reproducible)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int nparts, int n, float* __restrict__ dW,
                                                           int accumulate)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += part[(size_t)p * n + i];
    dW[i] = accumulate ? dW[i] + s : s;
}

}  // namespace ic3

// ---- ic3_comm_backward -------------------------------------------------------------------------------------------------------
extern "C" int ic3_comm_backward_partials(int E, int N)
{
    if (E <= 0 || N <= 0 || N > 64) return 0;
    const int ept = 64 / N, tiles = (E + ept - 1) / ept;
    constexpr int cap = 512;
    // at most 512 workgroups (two per CU; 768 / 1024 slots measured: 109 M against 111 M agent-steps/s per PP-hard update), every one
    // the same number of tiles: the launch lasts as long as the workgroup with the most tiles either way, and every workgroup fewer
    // is 2 x H x H x 4 bytes of partial sums less to add to (a chain of 4096 envs of 10 agents: 683 tiles as 342 x 2, not 171 x 2 + 341 x 1)
    const int rounds = (tiles + cap - 1) / cap;
    return (tiles + rounds - 1) / rounds;
}

extern "C" int ic3_comm_backward(const float* dxh, int ldd, const float* h_prev, const int32_t* alive, const int32_t* gate,
                                 const float* c_weight, const float* out_scale, float* dh_out,
                                 float* dcw_partials, int accumulate, int E, int N, int H, int mode_avg, int comm_zero,
                                 ic3_stream stream)
{
    using namespace ic3;
    if (!dxh || !dh_out || E <= 0 || N <= 0) return fail(-22, "ic3_comm_backward: null argument");
    if (ldd < 2 * H || (ldd & 3) || (H & 3)) return fail(-22, "ic3_comm_backward: ldd a multiple of 4, >= 2 * hid_size");
    hipStream_t s = (hipStream_t)stream;
    if (comm_zero) {                                             // no communication: the gate product's share alone
        const long long R = (long long)E * N, n4 = R * (H / 4);
        const int blocks = (int)std::min<long long>((n4 + 255) / 256, 4096);
        return launch_kernel(dh_copy_kernel, dim3(blocks), dim3(256), 0, s, dxh, ldd, out_scale, dh_out, R, H / 4);
    }
    if (!h_prev || !c_weight || !dcw_partials) return fail(-22, "ic3_comm_backward: null argument");
    if (H != 64 && H != 128 && H != 256) return fail(-38, "ic3_comm_backward: hid_size 64 / 128 / 256");
    if (N > 64) return fail(-38, "ic3_comm_backward: at most 64 agents per env");
    const int ept = 64 / N, tiles = (E + ept - 1) / ept;
    if ((long long)64 * ldd * 4 >= (1ll << 31)) return fail(-22, "ic3_comm_backward: row stride too large");
    const CommBwdArgs a{ dxh, h_prev, alive, gate, c_weight, out_scale, dh_out, dcw_partials, ldd, E, N, ept, tiles,
                         mode_avg, accumulate };
    const int grid = ic3_comm_backward_partials(E, N);
    const size_t lds = ((size_t)64 * (H + 4) + 128) * sizeof(float);
    // (at 256 one 512-thread workgroup per CU — dC's 8 accumulator blocks per wave live across the tiles — so the 512 workgroups
    //  of a large chain run as two rounds)
    const auto kernel = H == 256 ? comm_bwd_kernel<256> : H == 128 ? comm_bwd_kernel<128> : comm_bwd_kernel<64>;
    const int rc = launch_kernel(kernel, dim3(grid), dim3(2 * H), lds, s, a);
    return rc < 0 ? rc : grid;     // rows of dcw_partials written
}

// ---- ic3_lstm_weight_grad ----------------------------------------------------------------------------------------------------
// The K slices of a weight gradient over Q rows, `ny` workgroups per slice: two workgroups per CU, no slice under one 16-row
// stage, `per` rows per slice (a multiple of 16).  fits: `per` rows of `row_floats` floats stay below 2 GB — the kernels' 32-bit
// buffer offsets.
struct WGradPlan {
    int ks;
    long long per;
    bool fits;
};
static WGradPlan wgrad_plan(long long Q, int ny, long long row_floats)
{
    int ks = 2 * ic3::device_cus() / ny;
    const long long most = (Q + 15) / 16;
    if (ks > most) ks = (int)most;
    if (ks < 1) ks = 1;
    const long long per = ((Q + ks - 1) / ks + 15) / 16 * 16;
    return WGradPlan{ ks, per, per * row_floats * 4 < (1ll << 31) };
}

// dW (n floats) += / = the ks partials in `scratch`, summed in slice order; returns ks
static int wgrad_reduce(const float* scratch, int ks, int n, float* dW, int accumulate, hipStream_t s)
{
    const int rc = ic3::launch_kernel(ic3::wgrad_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, scratch, ks, n, dW, accumulate);
    return rc < 0 ? rc : ks;
}

// The plans at hid 256 (`ny` workgroups per slice — the LSTM's: 16): config 5's window is 80 x 262 144 rows of 4 KB, and a one-round slice of it lies
// past the kernels' 32-bit buffer offsets.  ks grows in whole multiples of the one-round count until a slice fits; the slices
// beyond the workgroup slots run as further rounds (the kernels know nothing of rounds).  64 / 128: wgrad_plan as it is.
// (Rounds of at least 8 slices: with fewer than 8 / ny CUs' worth of workgroup slots the plan is wgrad_plan's.)
static WGradPlan wgrad_plan_rounds(long long Q, int ny, long long row_floats)
{
    WGradPlan pl = wgrad_plan(Q, ny, row_floats);
    const long long most = (Q + 15) / 16;
    const int round = pl.ks;
    for (long long m = 2; !pl.fits && round * m <= most; ++m) {
        pl.ks = (int)(round * m);
        pl.per = ((Q + pl.ks - 1) / pl.ks + 15) / 16 * 16;
        pl.fits = pl.per * row_floats * 4 < (1ll << 31);
    }
    return pl;
}
static WGradPlan lstm_wgrad_plan(long long Q, int H, long long row_floats)
{
    return H == 256 ? wgrad_plan_rounds(Q, 16, row_floats) : wgrad_plan(Q, 4 * H / 128, row_floats);
}
// ic3_rnn_weight_grad: one workgroup per slice at 64 / 128; at 256 the four output quadrants of a slice, and further rounds as above
static WGradPlan rnn_wgrad_plan(long long Q, int H, long long row_floats)
{
    return H == 256 ? wgrad_plan_rounds(Q, 4, row_floats) : wgrad_plan(Q, 1, row_floats);
}

// ic3_lstm_weight_grad (hid 64 / 128) and ic3_lstm_weight_grad_wide (64 / 128 / 256) behind their hid_size checks
static int lstm_weight_grad(const float* inp, int ldi, const float* h_prev, const float* dgates, const float* row_live, long long Q,
                            int H, float* dW, int accumulate, int split, float* scratch, ic3_stream stream)
{
    using namespace ic3;
    if (!inp || !h_prev || !dgates || !dW || !scratch || Q <= 0) return fail(-22, "ic3_lstm_weight_grad: null argument");
    if (ldi < H || (ldi & 3)) return fail(-22, "ic3_lstm_weight_grad: ldi a multiple of 4, >= hid_size");
    const WGradPlan pl = lstm_wgrad_plan(Q, H, std::max(ldi, 4 * H));
    if (!pl.fits) return fail(-22, "ic3_lstm_weight_grad: a K slice must stay below 2 GB per operand (32-bit buffer offsets)");
    const WGradArgs a{ inp, h_prev, dgates, row_live, scratch, Q, ldi, (int)pl.per };
    hipStream_t s = (hipStream_t)stream;
    // split: exact bf16 split products (the rollout's arithmetic), two stages of 3 planes x 2 k halves of 16-byte fragments;
    // else the fp32 instruction on two stages of 16 rows.  Hid 256: the tile of 128, once per half of [inp | h] (grid z)
    const auto kernel = split ? (H == 256 ? lstm_wgrad_split_kernel<256> : H == 128 ? lstm_wgrad_split_kernel<128> : lstm_wgrad_split_kernel<64>)
                              : (H == 256 ? lstm_wgrad_kernel<256> : H == 128 ? lstm_wgrad_kernel<128> : lstm_wgrad_kernel<64>);
    const int HT = H == 256 ? 128 : H;
    const size_t lds = split ? (size_t)2 * 3 * 2 * (2 * HT + 128) * 16 : (size_t)2 * 16 * (2 * HT + 128) * sizeof(float);
    const dim3 grid = H == 256 ? dim3(pl.ks, 8, 2) : dim3(pl.ks, 4 * H / 128);
    if (const int rc = launch_kernel(kernel, grid, dim3(256), lds, s, a); rc < 0) return rc;
    return wgrad_reduce(scratch, pl.ks, 2 * H * 4 * H, dW, accumulate, s);
}

extern "C" size_t ic3_lstm_weight_grad_scratch_floats(long long Q, int H)
{
    if (Q <= 0 || (H != 64 && H != 128)) return 0;
    return (size_t)wgrad_plan(Q, 4 * H / 128, 0).ks * 2 * H * 4 * H;
}

extern "C" int ic3_lstm_weight_grad(const float* inp, int ldi, const float* h_prev, const float* dgates, const float* row_live,
                                    long long Q, int H, float* dW, int accumulate, int split, float* scratch, ic3_stream stream)
{
    if (H != 64 && H != 128) return ic3::fail(-38, "ic3_lstm_weight_grad: hid_size 64 / 128");
    return lstm_weight_grad(inp, ldi, h_prev, dgates, row_live, Q, H, dW, accumulate, split, scratch, stream);
}

extern "C" size_t ic3_lstm_weight_grad_wide_scratch_floats(long long Q, int H, int ldi)
{
    if (Q <= 0 || (H != 64 && H != 128 && H != 256)) return 0;
    return (size_t)lstm_wgrad_plan(Q, H, std::max(ldi, 4 * H)).ks * 2 * H * 4 * H;
}

extern "C" int ic3_lstm_weight_grad_wide(const float* inp, int ldi, const float* h_prev, const float* dgates, const float* row_live,
                                         long long Q, int H, float* dW, int accumulate, int split, float* scratch, ic3_stream stream)
{
    if (H != 64 && H != 128 && H != 256) return ic3::fail(-38, "ic3_lstm_weight_grad_wide: hid_size 64 / 128 / 256");
    return lstm_weight_grad(inp, ldi, h_prev, dgates, row_live, Q, H, dW, accumulate, split, scratch, stream);
}

// ---- ic3_bptt_backward -------------------------------------------------------------------------------------------------------
// The loop runs in place on the record (dgates over the gates): whatever could refuse a step is asked BEFORE the first one.
extern "C" int ic3_bptt_backward_supported(const ic3_env* env, int H)
{
    using namespace ic3;
    if (!env || (H != 64 && H != 128 && H != 256) || env->dims.N > 64) return 0;
    EncBwdPlan pl;
    if (env->kind == IC3_ENV_PP) {
        const ic3_pp_cfg& c = env->pp;
        const int W = 2 * c.vision + 1;
        pl = enc_bwd_plan(c.E, env->dims.N, c.N + c.nprey, H, c.dim * c.dim, 2 * W * W);
    } else {
        const ic3_tj_cfg& c = env->tj;
        const int WW = env->dims.window * env->dims.window, hdr = c.vocab_type ? 4 : 2;
        pl = enc_bwd_plan(c.E, c.N, c.N, H, env->dims.grid_h * env->dims.grid_w, hdr + WW);
    }
    return pl.csplit ? 1 : 0;     // (the sparse encoder's backward in its partial-sums form: ic3_env_encode_backward_accumulate)
}

namespace ic3 {
// the second chain's stream + the fork / join events, per device
struct BpttSide {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool ready = false;
};
static BpttSide* bptt_side()
{
    static BpttSide side[65];                                    // (slot 0: device -1, the host build's stand-in runtime)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < -1 || dev >= 64) return nullptr;
    BpttSide& sd = side[dev + 1];
    if (!sd.ready) {
        if (!sd.stream && hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if ((!sd.fork && hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming) != hipSuccess) ||
            (!sd.join && hipEventCreateWithFlags(&sd.join, hipEventDisableTiming) != hipSuccess))
            return nullptr;
        sd.ready = true;
    }
    return &sd;
}

// How a window call (`fn`, descriptor `B` = `sname`) opens: the struct_size handshake, T / E / N against the handle, what the
// configuration must be (`supported`, else -38 with `needs`), the heads' width.  ot_enosys: more than 16 columns is -38 of its own.
template <class B>
static int window_open(const char* fn, const char* sname, const ic3_env* env, const B* b, int (*supported)(const ic3_env*, int),
                       const char* needs, bool ot_enosys)
{
    const std::string f = std::string(fn) + ": ";
    if (!env || !b) return fail(-22, f + "null argument");
    if (b->struct_size != sizeof(B))
        return fail(-22, f + sname + " has " + std::to_string(b->struct_size) + " bytes, this library's has " +
                             std::to_string(sizeof(B)) + " (header / library version mismatch)");
    if (b->T <= 0 || b->E <= 0 || b->N <= 0 || b->E != env->dims.E || b->N != env->dims.N)
        return fail(-22, f + "T, E, N must be positive and E, N the handle's");
    if (!supported(env, b->H)) return fail(-38, f + needs);
    if (ot_enosys) {
        if (b->OT < 1) return fail(-22, f + "OT >= 1");
        if (b->OT > 16) return fail(-38, f + "at most 16 output columns");
    } else if (b->OT < 1 || b->OT > 16) {
        return fail(-22, f + "1 <= OT <= 16");
    }
    return 0;
}

// The sparse encoder's backward stage 1 behind a window's steps, over the T input gradients g + t * g_step: its window form (one
// launch), or its per-step form, last step first (the order of the per-step loops), `enc_first` cleared after the first.
static int encoder_tail(ic3_env* env, const int32_t* snaps, int64_t snap_words, int T, const float* g, int ldg, int64_t g_step,
                        int H, float* work, int enc_first, bool window, ic3_stream stream)
{
    if (window) return ic3_env_encode_backward_window(env, snaps, snap_words, T, g, ldg, g_step, H, work, enc_first, stream);
    for (int t = T - 1; t >= 0; --t) {
        const int rc = ic3_env_encode_backward_accumulate(env, snaps + (size_t)t * snap_words, g + (size_t)t * g_step, ldg, H, work,
                                                          enc_first, stream);
        if (rc < 0) return rc;
        enc_first = 0;
    }
    return 0;
}

// One LSTM cell of a window's backward on the rows of Ec envs — what ic3_bptt_backward issues per (step, chain) and
// its passes form (an ic3_bptt_passes descriptor) per (step, pass): ic3_lstm_gates_backward_given in place on the cell's gate record (the heads' share where
// dhead is given; `cut`: nothing arrives through dh / dc), then ic3_comm_backward, which leaves in dh what the cell in front receives.
struct BpttCell {
    float* gates;
    const float* c_prev;
    const float* h_prev;
    float* dh;
    float* dc;
    bool cut;
    float* dxh;
    float* dbias;
    const float* row_live;
    const float* row_keep;
    const float* dhead;
    const float* w_heads;
    int OT;
    const void* lstm_wp3_bwd;
    const int32_t* alive;
    const int32_t* gate;
    const float* c_weight;
    const float* out_scale;
    float* dcw;
    hipEvent_t ev0, ev1;                                         // recorded in front of / behind the gate launch, or null
};
static int bptt_cell_backward(const char* fn, const BpttCell& q, int Ec, int N, int H, int mode_avg, int comm_zero, hipStream_t sc)
{
    ic3_stream scv = (ic3_stream)sc;
    if (q.ev0 && hipEventRecord(q.ev0, sc) != hipSuccess) return fail(-5, std::string(fn) + ": hipEventRecord of a gate event failed");
    int rc = ic3_lstm_gates_backward_given(q.gates, nullptr, 0, nullptr, q.lstm_wp3_bwd, q.c_prev, q.cut ? nullptr : q.dh,
                                           q.cut ? nullptr : q.dc, q.gates, q.dc, q.dbias, 1, q.dxh, q.row_live, q.row_keep, q.dhead,
                                           q.dhead ? q.w_heads : nullptr, q.OT, Ec * N, H, scv);
    if (rc < 0) return rc;
    if (q.ev1 && hipEventRecord(q.ev1, sc) != hipSuccess) return fail(-5, std::string(fn) + ": hipEventRecord of a gate event failed");
    return ic3_comm_backward(q.dxh, 2 * H, q.h_prev, q.alive, q.gate, q.c_weight, q.out_scale, q.dh, q.dcw, 1, Ec, N, H, mode_avg,
                             comm_zero, scv);
}
}  // namespace ic3

// ---- ic3_bptt_backward on an ic3_bptt_passes descriptor ----------------------------------------------
// comm_passes = P > 1 (comm.py:179-218): a step is P chained LSTM cells on one snapshot, one pair of masks and one encoder output;
// pass i has its own C_i, only the last pass feeds the heads, only pass 0 touches the previous step.  The backward of a pass is the
// cell ic3_bptt_backward issues per step (bptt_cell_backward), on the records the recording ic3_policy_forward left: for t = T - 1 .. 0,
// i = P - 1 .. 0 — dhead on the last pass only, a detach point cuts what arrives at the last pass only, the communication backward
// of pass i leaves in dh what pass i - 1 (step t - 1 for i = 0) receives.  The encoder is linear in its input gradient, which is the
// sum of the passes' d inp: its window stage runs once per pass over that pass's ring and accumulates.
// Collection mode (row_keep / keep_before): dc flows uncut between the passes of one step and dh between them unscaled — the cuts sit
// on the slot's border alone.  The zero state entering a starting env is the caller's (zeroed copies as pass 0's hs / cs): no row_live.
static int bptt_passes_backward(ic3_env* env, const ic3_bptt_passes* b, ic3_stream stream)
{
    using namespace ic3;
    if (const int rc = window_open("ic3_bptt_backward (ic3_bptt_passes)", "ic3_bptt_passes", env, b, ic3_bptt_backward_supported,
                                   "hid_size 64 / 128 / 256, <= 64 agents, a grid whose encoder backward runs in its partial-sums form",
                                   false);
        rc < 0)
        return rc;
    const int T = b->T, E = b->E, N = b->N, H = b->H, P = b->passes;
    if (P < 2) return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): passes >= 2 (one pass: ic3_bptt_backward)");
    if (ic3_env_encode_backward_window_work(env, H) <= 0)
        return fail(-38, "ic3_bptt_backward (ic3_bptt_passes): needs a configuration with ic3_env_encode_backward_window (the ring form)");
    if (!b->gates || !b->hs || !b->cs || !b->dhead || !b->snaps || !b->lstm_wp3_bwd || !b->w_heads || !b->dh || !b->dc || !b->dxh ||
        !b->dbias_partials || !b->enc_work || b->t_first < 0)
        return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): null argument");
    if (!b->comm_zero && (!b->c_weight || !b->dcw_partials)) return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): the passes' C.weight and partials");
    const long long R = (long long)E * N;
    if (b->dxh_step < R * 2 * H) return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): dxh_step >= E * N * 2 * hid_size (the ring form)");
    for (int i = 0; i < P; ++i) {
        if (!b->gates[i] || !b->hs[i] || !b->cs[i] || !b->dxh[i] || !b->dbias_partials[i] ||
            (!b->comm_zero && (!b->c_weight[i] || !b->dcw_partials[i])))
            return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): null argument of pass " + std::to_string(i));
    }
    // (the loop runs in place on the records: what a launch would refuse is refused here, before the first one)
    if (R * 4 * H * 4 >= (1ll << 32))
        return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): rows * 4 * hid_size floats must stay below 4 GB (the gate launch's 32-bit buffer "
                         "offsets)");
    if (b->detach_gap > 0 && (b->row_keep || b->keep_before))
        return fail(-22, "ic3_bptt_backward (ic3_bptt_passes): detach_gap > 0 with row_keep / keep_before (a detached step has no dc for "
                         "row_keep to scale: lock-step windows carry detach_gap, collection-mode windows the row factors)");
    hipStream_t s = (hipStream_t)stream;
    for (int t = T - 1; t >= 0; --t) {
        const bool detached = b->detach_gap > 0 && (b->t_first + t + 1) % b->detach_gap == 0;
        // collection mode: what LEAVES slot t is cut by keep[t] — dc where it arrives, at the slot's last pass; dh where it is produced,
        // by pass 0 of slot t + 1 (so this slot's pass 0 scales by the keep row of the slot in front: keep_before at the call's first)
        const float* keep_here = b->row_keep ? b->row_keep + (size_t)t * R : nullptr;
        const float* keep_front = t > 0 ? (b->row_keep ? b->row_keep + (size_t)(t - 1) * R : nullptr) : b->keep_before;
        for (int i = P - 1; i >= 0; --i) {
            const bool last = i == P - 1;
            BpttCell q{};
            q.gates = b->gates[i] + (size_t)t * R * 4 * H;
            q.c_prev = b->cs[i] + (size_t)t * R * H;
            q.h_prev = b->hs[i] + (size_t)t * R * H;
            q.dh = b->dh;
            q.dc = b->dc;
            q.cut = detached && last;
            q.dxh = b->dxh[i] + (size_t)t * (size_t)b->dxh_step;
            q.dbias = b->dbias_partials[i];
            q.dhead = last ? b->dhead + (size_t)t * R * b->OT : nullptr;
            q.w_heads = b->w_heads;
            q.OT = b->OT;
            q.lstm_wp3_bwd = b->lstm_wp3_bwd;
            q.alive = (b->alive && b->alive[t]) ? b->alive[t] : nullptr;
            q.gate = (b->gate && b->gate[t]) ? b->gate[t] : nullptr;
            q.c_weight = b->comm_zero ? nullptr : b->c_weight[i];
            q.dcw = b->comm_zero ? nullptr : b->dcw_partials[i];
            q.row_keep = last ? keep_here : nullptr;
            q.out_scale = i == 0 ? keep_front : nullptr;
            if (const int rc = bptt_cell_backward("ic3_bptt_backward (ic3_bptt_passes)", q, E, N, H, b->mode_avg, b->comm_zero, s); rc < 0) return rc;
        }
    }
    for (int i = 0; i < P; ++i) {
        const int rc = ic3_env_encode_backward_window(env, b->snaps, b->snap_words, T, b->dxh[i], 2 * H, b->dxh_step, H, b->enc_work,
                                                      (i == 0 && b->enc_first) ? 1 : 0, stream);
        if (rc < 0) return rc;
    }
    return 0;
}

// ---- ic3_bptt_backward on an ic3_bptt_walk descriptor -------------------------------------------------
// A comm_zero window (IRIC's LSTM cell on its stand-in, --comm_mask_zero policies): the 2 T launches of the loop below — gate launch,
// then the copy of the d h_prev half — as ONE launch of lstm_gates_bwd_walk_kernel (gates_bwd.hip), then the encoder's window stage
// over the ring exactly as the loop issues it.  One stream.  Everything that could refuse is asked before the launch.
static int bptt_walk_backward(ic3_env* env, const ic3_bptt_walk* b, ic3_stream stream)
{
    using namespace ic3;
    const char* const fn = "ic3_bptt_backward (ic3_bptt_walk)";
    const std::string f = std::string(fn) + ": ";
    if (const int rc = window_open(fn, "ic3_bptt_walk", env, b, ic3_bptt_backward_supported,
                                   "hid_size 64 / 128 / 256, <= 64 agents, a grid whose encoder backward runs in its partial-sums form",
                                   false);
        rc < 0)
        return rc;
    if (!b->gates || !b->hs || !b->cs || !b->dhead || !b->snaps || !b->lstm_wp3_bwd || !b->w_heads || !b->dh || !b->dc || !b->dxh ||
        !b->dbias_partials || !b->enc_work)
        return fail(-22, f + "null argument");
    const long long R = (long long)b->E * b->N;
    if (b->dxh_step < R * 2 * b->H || ic3_env_encode_backward_window_work(env, b->H) <= 0)
        return fail(-22, f + "dxh_step >= E * N * 2 * hid_size, on a configuration with ic3_env_encode_backward_window (the walk needs "
                             "the ring)");
    if (b->detach_gap > 0 && b->row_keep)
        return fail(-22, f + "detach_gap > 0 with row_keep (a detached step has no dc for row_keep to scale: lock-step windows carry "
                             "detach_gap, collection-mode windows row_live / row_keep)");
    if (R >= (1ll << 31) || b->max_workgroups < 0) return fail(-22, f + "R < 2^31, max_workgroups >= 0");
    if (const int rc = lstm_gates_backward_walk(b, stream); rc < 0) return rc;
    return ic3_env_encode_backward_window(env, b->snaps, b->snap_words, b->T, b->dxh, 2 * b->H, b->dxh_step, b->H, b->enc_work,
                                          b->enc_first, stream);
}

// envs [0, E1) run on the caller's stream, [E1, E) on the library's second stream (ic3_bptt.two_chains): E1 * N a multiple of 64,
// so that the gate launch's row tiles — and with them its bias partials — do not straddle the border
extern "C" int ic3_bptt_first_chain_envs(int E, int N)
{
    if (E < 128 || N <= 0) return E;
    return (E / 2) & ~63;
}

extern "C" int ic3_bptt_backward(ic3_env* env, const ic3_bptt* b, ic3_stream stream)
{
    using namespace ic3;
    // (both descriptors start with struct_size; the passes form carries its magic in the next word, where an ic3_bptt holds T.  A
    //  tagged descriptor must have the passes struct's size exactly (window_open refuses it otherwise); an untagged one is an ic3_bptt)
    static_assert(offsetof(ic3_bptt_passes, magic) == offsetof(ic3_bptt, T), "the tag sits where ic3_bptt holds T");
    if (b && (uint32_t)b->T == IC3_BPTT_PASSES_MAGIC)
        return bptt_passes_backward(env, reinterpret_cast<const ic3_bptt_passes*>(b), stream);
    // (likewise the walk of a comm_zero window: its own tag, and a size that neither of the other two descriptors has)
    static_assert(offsetof(ic3_bptt_walk, magic) == offsetof(ic3_bptt, T), "the tag sits where ic3_bptt holds T");
    static_assert(sizeof(ic3_bptt_walk) != sizeof(ic3_bptt) && sizeof(ic3_bptt_walk) != sizeof(ic3_bptt_passes),
                  "the descriptors are told apart by their sizes too");
    if (b && (uint32_t)b->T == IC3_BPTT_WALK_MAGIC) return bptt_walk_backward(env, reinterpret_cast<const ic3_bptt_walk*>(b), stream);
    if (const int rc = window_open("ic3_bptt_backward", "ic3_bptt", env, b, ic3_bptt_backward_supported,
                                   "hid_size 64 / 128 / 256, <= 64 agents, a grid whose encoder backward runs in its partial-sums form",
                                   false);
        rc < 0)
        return rc;
    const int T = b->T, E = b->E, N = b->N, H = b->H;
    if (!b->gates || !b->hs || !b->cs || !b->dhead || !b->snaps || !b->lstm_wp3_bwd || !b->w_heads || !b->dh || !b->dc || !b->dxh ||
        !b->dbias_partials || !b->enc_work)
        return fail(-22, "ic3_bptt_backward: null argument");
    if (!b->comm_zero && (!b->c_weight || !b->dcw_partials)) return fail(-22, "ic3_bptt_backward: C.weight and its partials");
    if (b->dxh_step && (b->dxh_step < (long long)E * N * 2 * H || ic3_env_encode_backward_window_work(env, H) <= 0))
        return fail(-22, "ic3_bptt_backward: dxh_step >= E * N * 2 * hid_size, on a configuration with ic3_env_encode_backward_window");
    // (the loop runs in place on the record: what a step's launches would refuse is refused here, before the first one)
    if (b->detach_gap > 0 && b->row_keep)
        return fail(-22, "ic3_bptt_backward: detach_gap > 0 with row_keep (a detached step has no dc for row_keep to scale: lock-step "
                         "windows carry detach_gap, collection-mode windows row_live / row_keep)");
    const long long R = (long long)E * N;
    hipStream_t s = (hipStream_t)stream;
    // Two chains: the steps of envs [0, E1) and [E1, E) are independent until the weight gradients are summed, so with
    // two_chains their launches go to two streams and the GPU fills the ragged last round of one chain's launch (1280 row tiles
    // on 512 workgroup slots = 2.5 rounds at PP-hard E = 8192) with the other chain's workgroups.  Needs what ties the chains
    // together to be per step or behind the loop: the ring of input gradients (the encoder's stage 1 behind the loop).
    const int E1 = (b->two_chains && b->dxh_step) ? ic3_bptt_first_chain_envs(E, N) : E;
    const int nch = E1 < E ? 2 : 1;
    if ((long long)std::max(E1, E - E1) * N * 4 * H * 4 >= (1ll << 32))
        return fail(-22, "ic3_bptt_backward: a chain's rows * 4 * hid_size floats must stay below 4 GB (the gate launch's 32-bit buffer "
                         "offsets)");
    BpttSide* side = nch == 2 ? bptt_side() : nullptr;
    if (nch == 2 && !side) return fail(-12, "ic3_bptt_backward: no second stream");
    if (nch == 2) {
        IC3_HIP(hipEventRecord(side->fork, s));
        IC3_HIP(hipStreamWaitEvent(side->stream, side->fork, 0));
    }
    // an error behind the fork still joins the second stream: the caller's stream must not run ahead of launches that read its buffers
    auto join = [&](int rc) {
        if (nch == 2 && (hipEventRecord(side->join, side->stream) != hipSuccess || hipStreamWaitEvent(s, side->join, 0) != hipSuccess) &&
            rc >= 0)
            return fail(-5, "ic3_bptt_backward: joining the second stream failed");
        return rc;
    };
    int enc_first = b->enc_first;
    for (int t = T - 1; t >= 0; --t) {
        for (int ch = 0; ch < nch; ++ch) {
            const int e0 = ch ? E1 : 0, Ec = ch ? E - E1 : E1;
            const size_t r0 = (size_t)e0 * N;
            hipStream_t sc = ch ? side->stream : s;
            // trainer.py:56-60: (h_t, c_t) were handed on detached — the gate launch reads zeros for dL/d(h_t, c_t) (null inputs: an
            // empty descriptor instead of two memsets and their reads)
            const bool detached = b->detach_gap > 0 && (t + 1) % b->detach_gap == 0;
            BpttCell q{};
            q.gates = b->gates + ((size_t)t * R + r0) * 4 * H;
            q.c_prev = b->cs + ((size_t)t * R + r0) * H;
            q.h_prev = b->hs + ((size_t)t * R + r0) * H;
            q.dh = b->dh + r0 * H;
            q.dc = b->dc + r0 * H;
            q.cut = detached;
            q.dxh = b->dxh + (size_t)t * (size_t)b->dxh_step + r0 * 2 * H;
            q.dbias = b->dbias_partials + (r0 / 64) * 4 * H;
            q.row_live = b->row_live ? b->row_live + (size_t)t * R + r0 : nullptr;
            q.row_keep = b->row_keep ? b->row_keep + (size_t)t * R + r0 : nullptr;
            q.dhead = b->dhead + ((size_t)t * R + r0) * b->OT;
            q.w_heads = b->w_heads;
            q.OT = b->OT;
            q.lstm_wp3_bwd = b->lstm_wp3_bwd;
            q.alive = (b->alive && b->alive[t]) ? b->alive[t] + r0 : nullptr;
            q.gate = (b->gate && b->gate[t]) ? b->gate[t] + r0 : nullptr;
            q.c_weight = b->c_weight;
            q.out_scale = (b->row_keep && t > 0) ? b->row_keep + (size_t)(t - 1) * R + r0 : nullptr;
            q.dcw = b->dcw_partials;
            if (q.dcw && ch) q.dcw += (size_t)ic3_comm_backward_partials(E1, N) * H * H;
            if (b->gate_events && ch == 0) {
                q.ev0 = (hipEvent_t)b->gate_events[2 * t];
                q.ev1 = (hipEvent_t)b->gate_events[2 * t + 1];
            }
            const int rc = bptt_cell_backward("ic3_bptt_backward", q, Ec, N, H, b->mode_avg, b->comm_zero, sc);
            if (rc < 0) return join(rc);
        }
        if (b->dxh_step) continue;                               // (the encoder's first stage: once, behind the loop)
        int rc = ic3_env_encode_backward_accumulate(env, b->snaps + (size_t)t * b->snap_words, b->dxh, 2 * H, H, b->enc_work,
                                                    enc_first, stream);
        if (rc < 0) return join(rc);
        enc_first = 0;
    }
    if (const int rc = join(0); rc < 0) return rc;
    if (b->dxh_step)
        return ic3_env_encode_backward_window(env, b->snaps, b->snap_words, T, b->dxh, 2 * H, b->dxh_step, H, b->enc_work, enc_first,
                                              stream);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// ic3_rnn_backward: the IC / IRIC baselines' tanh recurrence (models.py:68-92, rnn_type 'MLP'),
//     h_t = tanh(affine1(obs_t) + affine2(h_{t-1})),   [logits | value]_t = W_heads h_t + b,
// differentiated over a window of recorded steps, last to first.  Per step ONE launch (rnn_tanh_bwd_kernel):
//     dh_t   = dh_in + d_t . W_heads                      (dh_in: what step t + 1 sent back; zeros at a detach point)
//     dz_t   = dh_t * (1 - h_t^2)                          -> the ring slot t (the affine1 / affine2 pre-activation gradient)
//     dh_out = (dz_t . A2) * out_scale                     (A2 = affine2.weight; out_scale = row_keep[t - 1] in collection mode)
//     per-workgroup column sums of dz_t                    (d affine1.bias = d affine2.bias; fixed-order reduction by the caller)
// and behind the loop ONE launch for dA2 += sum_t dz_t^T . (row_live_t h_{t-1}) over all T x R rows (rnn_wgrad_kernel).
//
// rnn_tanh_bwd_kernel<H>: 4H threads (H / 8 waves), persistent over tiles of 64 rows.  A2 sits in LDS for the workgroup's life,
// in fragment order: float4 (kb, hi, col) = A2[8 kb + 4 hi + j][col], j = 0..3 — the B operand of four 32 x 32 x 2 MFMAs is one
// conflict-free ds_read_b128.  Per tile: phase 0 — thread (row group, 4-column chunk) forms dz for 4 rows (its W_heads chunk and
// the tile's d rows from LDS), writes it to the ring and to the LDS tile, adds it to its column sums; phase 1 — wave (rb, cb)
// multiplies tile rows [32 rb, +32) by A2's columns [32 cb, +32) and writes dh_out.  dh_out may be dh_in: a workgroup reads all
// of its tile's dh_in rows before the barrier in front of the product, and no other workgroup touches those rows.
// LDS: H^2 + 64 (H + 4) + 16 H + 1024 floats (110 KB at H = 128: one workgroup of 8 waves per CU; 41 KB at 64: two of 4).
// HBM per row: dh_in, h_t in, dz, dh_out out (4 H floats) + OT; MFMA 2 H^2 flop per row on the fp32 instruction.
//
// H = 256 — the plan: A2 STREAMED FROM L2, rows owned by one workgroup.  A2 is 256 KB, more than a CU's 160 KB of LDS, so
// rnn_tanh_bwd_kernel<256> / mlp_bwd_kernel<256> keep the same tile machine (1024 threads = 16 waves, a 64-row tile, wave (rb, cb) =
// 32 rows x 32 of the 256 columns, phase 0 / product / epilogue unchanged) and only TanhTile<256>::product differs: a lane's B values
// A2[k][col] come from global memory through a buffer descriptor, 8 loads (16 k rows) per stage, the next stage requested in front
// of this stage's 8 MFMAs.  All workgroups read the same 256 KB, which stays in every XCD's L2.  Staging 64-column chunks of A2
// through LDS per tile moves the same 256 KB per tile from L2 and adds an LDS round trip and four barriers per tile, so it was not
// taken.  A workgroup owns ALL 256 columns of its tile's rows (phase 0 reads every dh_in row of the tile in front of the barrier
// before the product): dh_out == dh_in stays legal.  No atomics; the column sums are the row groups' sums in group order, as at
// 64 / 128.
// LDS: 64 (H + 4) + 16 H + 1024 floats = 87 040 bytes: one workgroup of 16 waves per CU (4 per SIMD, <= 128 registers each).
// Per row: HBM dh_in, h_t in, dz, dh_out out = 4 KB (+ OT floats; mlp: 5 KB); L2 16 waves x 32 KB of A2 per 64-row tile = 8 KB.
// ---------------------------------------------------------------------------------------------------------------------------
namespace ic3 {

// The tile machine of rnn_tanh_bwd_kernel and mlp_bwd_kernel: the constants, the LDS layout, a thread's two coordinates and the
// four pieces both kernels run unchanged.  What differs — the phase-0 arithmetic, what happens to the product, when the next
// tile's rows are requested — stays in the kernels.
template <int H>
struct TanhTile {
    static constexpr int NT = 4 * H, H4 = H / 4, LDA = H + 4, LDA4 = LDA / 4, CB = H / 32, RPP = NT / H4, PER = 64 / RPP;
    static_assert(RPP * PER == 64 && NT / 64 == 2 * CB, "tile split");
    // A2 in LDS for the workgroup's life (64 / 128), or — 256 KB at H = 256, more than a CU's LDS — its B fragments streamed from L2
    static constexpr bool RESIDENT = H <= 128;
    // LDS in floats: A2 in fragment order (RESIDENT) | the tile's dz | W_heads | the tile's d rows
    static constexpr int DZ_AT = RESIDENT ? H * H : 0, WH_AT = DZ_AT + 64 * LDA, SD_AT = WH_AT + 16 * H;
    static constexpr size_t LDS_BYTES = (size_t)(SD_AT + 64 * 16) * sizeof(float);
    float* const smem;
    const bp_f32x4* const Bf4;   // [H / 8][2][H] float4
    float* const Dz;             // [64][LDA]
    bp_f32x4* const Dz4;
    float* const Wh;             // [16][H]
    float* const Sd;             // [64][OT]
    const int tid, li, lh;
    const int cb, rb;            // the product: wave (rb, cb) = tile rows [32 rb, +32) x A2's columns [32 cb, +32)
    const int c4, rg;            // phase 0, column sums: column chunk c4 of rows rg + RPP i

    __device__ __forceinline__ explicit TanhTile(float* lds)
        : smem(lds), Bf4(reinterpret_cast<const bp_f32x4*>(lds)), Dz(lds + DZ_AT), Dz4(reinterpret_cast<bp_f32x4*>(lds + DZ_AT)),
          Wh(lds + WH_AT), Sd(lds + SD_AT), tid(threadIdx.x), li(threadIdx.x & 31), lh((threadIdx.x & 63) >> 5),
          cb((threadIdx.x >> 6) % CB), rb((threadIdx.x >> 6) / CB), c4(threadIdx.x % H4), rg(threadIdx.x / H4)
    {
    }
    // A2 -> fragment order (RESIDENT), W_heads as it is (the caller's barrier behind it)
    __device__ __forceinline__ void stage_weights(const float* a2, const float* w_heads, int OT) const
    {
        if constexpr (RESIDENT) {
            for (int i = tid; i < H * H; i += NT) {
                const int k = i / H, col = i - k * H;
                smem[(((k >> 3) * 2 + ((k >> 2) & 1)) * H + col) * 4 + (k & 3)] = a2[i];
            }
        }
        for (int i = tid; i < OT * H; i += NT) Wh[i] = w_heads[i];
    }
    // v + d[row] . W_heads for the thread's 4 columns
    __device__ __forceinline__ bp_f32x4 heads_share(bp_f32x4 v, int row, int OT) const
    {
        const bp_f32x4* const Wh4 = reinterpret_cast<const bp_f32x4*>(Wh);
        for (int o = 0; o < OT; ++o) v += Sd[row * OT + o] * Wh4[o * H4 + c4];
        return v;
    }
    // the wave's 32 x 32 block of dz . A2 on the fp32 matrix instruction (k = 8 kb + 4 lh + j: A fragment and B slot agree)
    // Streamed (H = 256): the lane's B values A2[8 kb + 4 lh + j][32 cb + li] come from global memory (L2: all workgroups read the
    // same 256 KB), 16 k rows = 8 loads per stage, the next stage requested in front of this one's 8 MFMAs (past A2's end: 0).
    __device__ __forceinline__ bp_f32x16 product(const float* a2) const
    {
        bp_f32x16 acc;
        bp_zero<1>(&acc);
        if constexpr (RESIDENT) {
#pragma unroll 4
            for (int kb = 0; kb < H / 8; ++kb) {
                const bp_f32x4 a4 = Dz4[(32 * rb + li) * LDA4 + 2 * kb + lh];
                const bp_f32x4 b4 = Bf4[(2 * kb + lh) * H + 32 * cb + li];
#pragma unroll
                for (int j = 0; j < 4; ++j) bp_mfma(acc, a4[j], b4[j]);
            }
        } else {
            const __amdgpu_buffer_rsrc_t ra = bp_rsrc(a2, (long long)H * H * 4);
            const int voff = (4 * lh * H + 32 * cb + li) * 4;
            float bv[8], bn[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = bp_load1(ra, voff, (8 * (j >> 2) + (j & 3)) * H * 4);
#pragma unroll 2
            for (int kb = 0; kb < H / 8; kb += 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) bn[j] = bp_load1(ra, voff, (8 * (kb + 2 + (j >> 2)) + (j & 3)) * H * 4);
                const bp_f32x4 a0 = Dz4[(32 * rb + li) * LDA4 + 2 * kb + lh];
                const bp_f32x4 a1 = Dz4[(32 * rb + li) * LDA4 + 2 * kb + 2 + lh];
#pragma unroll
                for (int j = 0; j < 4; ++j) bp_mfma(acc, a0[j], bv[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) bp_mfma(acc, a1[j], bv[4 + j]);
#pragma unroll
                for (int j = 0; j < 8; ++j) bv[j] = bn[j];
            }
        }
        return acc;
    }
    // column sums of the workgroup: the RPP row groups of a chunk added in group order (reproducible)
    __device__ __forceinline__ void column_sums(bp_f32x4 bsum, float* db_part, int accumulate) const
    {
        Dz4[rg * H4 + c4] = bsum;
        __syncthreads();
        if (tid < H4) {
            bp_f32x4 s = Dz4[tid];
            for (int g = 1; g < RPP; ++g) s += Dz4[g * H4 + tid];
            bp_f32x4* dst = reinterpret_cast<bp_f32x4*>(db_part + (size_t)blockIdx.x * H) + tid;
            *dst = accumulate ? *dst + s : s;
        }
    }
};

struct RnnBwdArgs {
    const float* dh_in;      // [R][H] or null (zeros)
    const float* h;          // [R][H] h_t
    const float* dhead;      // [R][OT]
    const float* w_heads;    // [OT][H]
    const float* a2;         // [H][H] affine2.weight (out, in): dh_out = dz . A2
    const float* out_scale;  // [R] or null
    float* dz;               // [R][H]
    float* dh_out;           // [R][H]
    float* db_part;          // [gridDim.x][H]
    int R, OT, tiles, accumulate;
};

template <int H>
__global__ __launch_bounds__(4 * H, (H <= 64) ? 2 : 1) void rnn_tanh_bwd_kernel(const RnnBwdArgs a)
{
    using Tile = TanhTile<H>;
    constexpr int NT = Tile::NT, LDA4 = Tile::LDA4, RPP = Tile::RPP, PER = Tile::PER;
    IC3_DYNAMIC_LDS(float, smem);
    const Tile t(smem);
    const int OT = a.OT;
    t.stage_weights(a.a2, a.w_heads, OT);
    bp_f32x4 bsum = { 0.f, 0.f, 0.f, 0.f };
    __syncthreads();
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * 64;
        const int rows = (a.R - r0) < 64 ? (int)(a.R - r0) : 64;
        // (rows past the tile read 0 and their stores are dropped: the ranges of the buffer descriptors)
        const __amdgpu_buffer_rsrc_t rdi = bp_rsrc(a.dh_in ? a.dh_in + r0 * H : a.h, a.dh_in ? (long long)rows * H * 4 : 0);
        const __amdgpu_buffer_rsrc_t rh = bp_rsrc(a.h + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rd = bp_rsrc(a.dhead + r0 * OT, (long long)rows * OT * 4);
        const __amdgpu_buffer_rsrc_t rz = bp_rsrc(a.dz + r0 * H, (long long)rows * H * 4);
        bp_f32x4 dv[PER], hv[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int off = ((t.rg + RPP * i) * H + 4 * t.c4) * 4;
            dv[i] = bp_load4(rdi, off);
            hv[i] = bp_load4(rh, off);
        }
        for (int i = t.tid; i < 64 * OT; i += NT) t.Sd[i] = bp_load1(rd, i * 4);
        __syncthreads();
        // ---- phase 0: dz of the tile -> ring, LDS, column sums
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int row = t.rg + RPP * i;
            const bp_f32x4 v = t.heads_share(dv[i], row, OT);
            const bp_f32x4 z = v * (1.0f - hv[i] * hv[i]);
            bsum += z;
            t.Dz4[row * LDA4 + t.c4] = z;
            bp_store4(z, rz, (row * H + 4 * t.c4) * 4);
        }
        __syncthreads();
        // ---- phase 1: dh_out = (dz . A2) * out_scale, stored from the accumulator layout
        const bp_f32x16 acc = t.product(a.a2);
        const __amdgpu_buffer_rsrc_t rout = bp_rsrc(a.dh_out + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rsc = bp_rsrc(a.out_scale ? a.out_scale + r0 : a.dh_out, a.out_scale ? (long long)rows * 4 : 0);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int lr = 32 * t.rb + (reg & 3) + 8 * (reg >> 2) + 4 * t.lh;
            float o = acc[reg];
            if (a.out_scale) o *= bp_load1(rsc, lr * 4);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, o), rout, (lr * H + 32 * t.cb + t.li) * 4, 0, 0);
        }
        __syncthreads();                                         // every wave is done with the tile's LDS
    }
    t.column_sums(bsum, a.db_part, a.accumulate);
}

// ---------------------------------------------------------------------------------------------------------------------------
// rnn_tanh_bwd_walk_kernel<H>: the T launches of rnn_tanh_bwd_kernel over a window as ONE (ic3_rnn_backward_wide on an
// ic3_rnn_bptt_walk descriptor).  No row's gradient depends on another row, so the workgroup that owns a 64-row tile walks
// t = T - 1 .. 0 by itself and finishes the tile's whole window before its next tile: no grid barrier, no flag, nothing that waits for
// another workgroup.  The tile machine, the phase-0 arithmetic, the product and the scaling are rnn_tanh_bwd_kernel's, element by
// element; A2 (64 / 128) and W_heads are staged once per launch, not once per step.
// Where dL/dh lives between the steps: in the Dz TILE — the epilogue writes (dz_t . A2) * row_keep[t - 1] over it from the accumulator
// layout behind a barrier of its own (every wave is done reading dz_t), the next step's phase 0 reads it back in the (row group,
// column chunk) layout and writes dz_{t-1} over its own slots.  Three barriers per step instead of two; taken over a second tile of
// 64 x (H + 4) floats because that tile, at hid 256, leaves no room in 160 KB for the column sums' 16 H floats (153.6 + 16 KB), and
// one layout serves the three sizes.  dh crosses HBM twice per tile: in from a.dh in front of the tile's first step (into the tile; a
// detached step reads zeros instead, as the per-step launch takes a null dh_in), out to a.dh behind step 0.
// Prefetch: the rows of h and dhead of step t - 1 and the row_keep factors of step t are requested in front of step t's product —
// none depends on dh.  Buffer descriptors per step from 64-bit tile bases (no launch-wide 32-bit limit: R < 2^31, OT <= 16).
// Bias partials: ONE ROW PER TILE, db_part [tiles][H].  Per step the thread sums over the thread's rows and their sum over the row
// groups in group order (column_sums' order), added to a running total that STARTS FROM row `tile` — step T - 1 first, the row
// written once behind step 0: the additions rnn_tanh_bwd_kernel makes to a workgroup's row over the T launches, in their order,
// whatever the row held (one tile per workgroup there: the same bits).
// LDS: TanhTile's + 16 H floats (the row groups' sums): 45 KB at 64 (two workgroups per CU), 117 KB at 128, 101 KB at 256 (one).
// HBM per row and step: h_t in, dz out (2 H floats) + OT (+ one row_keep float).
// ---------------------------------------------------------------------------------------------------------------------------
struct RnnWalkArgs {
    const float* hs;         // [>= T (+1)][R][H]: slot t + 1 = h_t
    const float* h_last;     // [R][H] or null: h_{T-1} when not slot T
    const float* dhead;      // [T][R][OT]
    const float* w_heads;    // [OT][H]
    const float* a2;         // [H][H]
    const float* row_keep;   // [T][R] or null
    float* dh;               // [R][H] in: arriving at step T - 1, out: leaving step 0
    float* dz;               // [T][R][H] the ring
    float* db_part;          // [tiles][H], added to
    int R, OT, tiles, T, detach_gap;
};

template <int H>
__global__ __launch_bounds__(4 * H, (H <= 64) ? 2 : 1) void rnn_tanh_bwd_walk_kernel(const RnnWalkArgs a)
{
    using Tile = TanhTile<H>;
    constexpr int NT = Tile::NT, H4 = Tile::H4, LDA4 = Tile::LDA4, RPP = Tile::RPP, PER = Tile::PER;
    constexpr int SDN = (64 * 16 + NT - 1) / NT;                 // dhead values of a tile per thread, at the widest heads
    IC3_DYNAMIC_LDS(float, smem);
    const Tile t(smem);
    bp_f32x4* const Gs4 = reinterpret_cast<bp_f32x4*>(smem + Tile::SD_AT + 64 * 16);   // [RPP][H4] the row groups' sums of a step
    const int OT = a.OT, T = a.T;
    const size_t R = (size_t)a.R;
    t.stage_weights(a.a2, a.w_heads, OT);
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * 64;
        const int rows = (a.R - r0) < 64 ? (int)(a.R - r0) : 64;
        // (rows past the tile read 0 and their stores are dropped: the ranges of the buffer descriptors)
        const long long hb = (long long)rows * H * 4;
        bp_f32x4 hv[PER];
        float sdv[SDN];
        auto request = [&](int s) {                              // step s: its rows of h and dhead -> registers
            const float* h_s = (s + 1 < T || !a.h_last) ? a.hs + (size_t)(s + 1) * R * H : a.h_last;
            const __amdgpu_buffer_rsrc_t rh = bp_rsrc(h_s + r0 * H, hb);
            const __amdgpu_buffer_rsrc_t rd = bp_rsrc(a.dhead + ((size_t)s * R + r0) * OT, (long long)rows * OT * 4);
#pragma unroll
            for (int i = 0; i < PER; ++i) hv[i] = bp_load4(rh, ((t.rg + RPP * i) * H + 4 * t.c4) * 4);
#pragma unroll
            for (int k = 0; k < SDN; ++k) sdv[k] = bp_load1(rd, (t.tid + k * NT) * 4);
        };
        request(T - 1);
        {   // dL/dh arriving at the window's last step -> the thread's own slots of the tile
            const __amdgpu_buffer_rsrc_t rdi = bp_rsrc(a.dh + r0 * H, hb);
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int row = t.rg + RPP * i;
                t.Dz4[row * LDA4 + t.c4] = bp_load4(rdi, (row * H + 4 * t.c4) * 4);
            }
        }
        bp_f32x4 total = { 0.f, 0.f, 0.f, 0.f };
        bp_f32x4* const prow = reinterpret_cast<bp_f32x4*>(a.db_part + (size_t)tile * H) + t.tid;
        if (t.tid < H4) total = *prow;
        for (int s = T - 1; s >= 0; --s) {
            const bool detached = a.detach_gap > 0 && (s + 1) % a.detach_gap == 0;
#pragma unroll
            for (int k = 0; k < SDN; ++k)
                if (t.tid + k * NT < 64 * OT) t.Sd[t.tid + k * NT] = sdv[k];
            __syncthreads();                                     // the step's d rows; what the epilogue left in the tile (the weights)
            // ---- phase 0: dz of the tile -> ring, LDS (over the thread's own slots of dL/dh), column sums
            const __amdgpu_buffer_rsrc_t rz = bp_rsrc(a.dz + ((size_t)s * R + r0) * H, hb);
            bp_f32x4 bsum = { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int row = t.rg + RPP * i;
                bp_f32x4 dv = { 0.f, 0.f, 0.f, 0.f };
                if (!detached) dv = t.Dz4[row * LDA4 + t.c4];
                const bp_f32x4 v = t.heads_share(dv, row, OT);
                const bp_f32x4 z = v * (1.0f - hv[i] * hv[i]);
                {   // (the ROUNDED dz is what is summed, as in the per-step kernel: this add must not be fused with the product above,
                    //  whatever the code around it invites the compiler to do)
#pragma clang fp contract(off)
                    bsum = bsum + z;
                }
                t.Dz4[row * LDA4 + t.c4] = z;
                bp_store4(z, rz, (row * H + 4 * t.c4) * 4);
            }
            Gs4[t.rg * H4 + t.c4] = bsum;
            __syncthreads();
            // ---- what does not wait for dh: the next step's rows, this step's factors, the step's column sums
            if (s > 0) request(s - 1);
            const bool scaled = a.row_keep && s > 0;
            float kv[16];
            if (scaled) {
                const __amdgpu_buffer_rsrc_t rsc = bp_rsrc(a.row_keep + (size_t)(s - 1) * R + r0, (long long)rows * 4);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) kv[reg] = bp_load1(rsc, (32 * t.rb + (reg & 3) + 8 * (reg >> 2) + 4 * t.lh) * 4);
            }
            if (t.tid < H4) {
                bp_f32x4 g = Gs4[t.tid];
                for (int j = 1; j < RPP; ++j) g += Gs4[j * H4 + t.tid];
                total = total + g;
            }
            // ---- phase 1: (dz . A2) * row_keep[s - 1] -> the tile (the next step's dL/dh), or behind step 0 -> a.dh
            const bp_f32x16 acc = t.product(a.a2);
            if (s > 0) {
                __syncthreads();                                 // every wave is done reading dz_s
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int lr = 32 * t.rb + (reg & 3) + 8 * (reg >> 2) + 4 * t.lh;
                    float o = acc[reg];
                    if (scaled) o *= kv[reg];
                    t.Dz[lr * Tile::LDA + 32 * t.cb + t.li] = o;
                }
            } else {
                const __amdgpu_buffer_rsrc_t rout = bp_rsrc(a.dh + r0 * H, hb);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int lr = 32 * t.rb + (reg & 3) + 8 * (reg >> 2) + 4 * t.lh;
                    const float o = acc[reg];
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, o), rout, (lr * H + 32 * t.cb + t.li) * 4, 0, 0);
                }
            }
        }
        if (t.tid < H4) *prow = total;
        __syncthreads();                                         // every wave is done with the tile's LDS
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ic3_rnn_weight_grad.  dA2[m][n] = sum_q dz[q][m] (row_live[q] h_prev[q][n]) over Q = T x R rows.  Workgroup = K slice of the
// rows, all H x H outputs; 4 waves as 2 (m) x 2 (n), a wave holds (H / 2) x (H / 2) of the result (MB x MB blocks of 32 x 32).
// Both operands row-major with q outermost — the K-major pair v_mfma_f32_32x32x2_f32 wants: lane (i, kk) supplies dz[q0 + kk][m(i)]
// and h[q0 + kk][n(i)].  Staging: KT = 16 rows of each per stage, global -> registers -> LDS, double-buffered, one barrier per
// stage (the shape of lstm_wgrad_kernel).  Bound: HBM (2 H floats per row) against MFMA (2 H^2 flop per row) — about even at 128.
// Hid 256: all H x H outputs in one workgroup would be 256 accumulator registers per wave, so <256> IS the tile of 128 (HT) on the
// four output quadrants — grid (ks, 2, 2), blockIdx.y picks the 128 dz columns (output rows), blockIdx.z the 128 h columns, both
// staged with the row stride of 256; row_live scales the h rows on the way in, as at 128.  The partials are [ks][256][256]; the K
// slices grow by whole rounds of workgroups until one stays below 2 GB (rnn_wgrad_plan).  WIDE / HT fold away at 64 / 128.
// ---------------------------------------------------------------------------------------------------------------------------
struct RnnWGradArgs {
    const float* dz;         // [Q][H]
    const float* h;          // [Q][H] h_prev
    const float* row_live;   // [Q] or null: h rows times it
    float* part;             // [gridDim.x][H][H]
    long long Q;
    int rows_per_wg;         // rows per K slice (a multiple of 16)
};

template <int H>
__global__ __launch_bounds__(256, 2) void rnn_wgrad_kernel(const RnnWGradArgs a)
{
    constexpr bool WIDE = H == 256;
    constexpr int HT = WIDE ? 128 : H;                           // the tile: HT dz columns x HT h columns of a row
    constexpr int KT = 16, NT = 256, H4 = HT / 4, MB = HT / 64, HH = HT / 2;
    constexpr int RPS = NT / H4, PT = KT / RPS;                  // rows staged per pass, passes per stage (2 at HT = 128, 1 at 64)
    constexpr int SW = 2 * KT * HT;                              // stage b: dz rows at smem + b * SW, h rows behind them
    static_assert(PT >= 1 && RPS * PT == KT, "staging split");
    IC3_DYNAMIC_LDS(float, smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = w & 1, wn = w >> 1;
    const int zc = WIDE ? HT * (int)blockIdx.y : 0, hc = WIDE ? HT * (int)blockIdx.z : 0;   // the quadrant's first dz / h column
    const KSlice sl = bp_kslice(a.Q, a.rows_per_wg, KT);
    const long long q0 = sl.q0, nq = sl.nq;
    const int nstages = sl.nstages;
    // (WIDE: HT columns of rows H floats apart — the range ends behind the last row's HT columns, so rows past the slice read 0)
    const __amdgpu_buffer_rsrc_t rz = bp_rsrc(nq > 0 ? a.dz + q0 * H + zc : a.dz, WIDE ? ((nq - 1) * H + HT) * 4 : nq * H * 4);
    const __amdgpu_buffer_rsrc_t rh = bp_rsrc(nq > 0 ? a.h + q0 * H + hc : a.h, WIDE ? ((nq - 1) * H + HT) * 4 : nq * H * 4);
    const __amdgpu_buffer_rsrc_t rl = bp_rsrc(a.row_live && nq > 0 ? a.row_live + q0 : a.h, a.row_live ? nq * 4 : 0);
    const int srow = tid / H4, sc4 = tid - srow * H4;            // a thread stages rows srow + RPS i, column chunk sc4
    bp_f32x4 zr[PT], hr[PT];
    auto fetch = [&](int s) {
        const int qb = s * KT;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int off = ((srow + RPS * i) * H + 4 * sc4) * 4;
            zr[i] = bp_load4(rz, off, qb * H * 4);
            hr[i] = bp_load4(rh, off, qb * H * 4);
            if (a.row_live) hr[i] *= bp_load1(rl, (srow + RPS * i) * 4, qb * 4);
        }
    };
    auto stash = [&](int b) {
        bp_f32x4* Z4 = reinterpret_cast<bp_f32x4*>(smem + b * SW);
        bp_f32x4* P4 = Z4 + KT * H4;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            Z4[tid + i * NT] = zr[i];
            P4[tid + i * NT] = hr[i];
        }
    };
    bp_f32x16 acc[MB][MB];
    bp_zero<MB * MB>(&acc[0][0]);
    if (nstages > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
        if (more) fetch(s + 1);
        const float* Zs = smem + (s & 1) * SW;
        const float* Ps = Zs + KT * HT;
#pragma unroll
        for (int ks = 0; ks < KT / 2; ++ks) {
            const int kr = 2 * ks + lh;
            float av[MB], bv[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                av[mb] = Zs[kr * HT + wm * HH + 32 * mb + li];
                bv[mb] = Ps[kr * HT + wn * HH + 32 * mb + li];
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < MB; ++nb) bp_mfma(acc[mb][nb], av[mb], bv[nb]);
        }
        if (more) stash((s + 1) & 1);
        __syncthreads();
    }
    // block (mb, nb), register reg, lane (li, lh): m = wm HT / 2 + 32 mb + (reg & 3) + 8 (reg >> 2) + 4 lh, n = wn HT / 2 + 32 nb + li
    float* dst = a.part + (size_t)blockIdx.x * H * H + (size_t)zc * H + hc;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < MB; ++nb)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int m = wm * HH + 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                dst[(size_t)m * H + wn * HH + 32 * nb + li] = acc[mb][nb][reg];
            }
}

}  // namespace ic3

// ---- ic3_rnn_backward --------------------------------------------------------------------------------------------------------
// Tile plan of a tanh kernel's launch over `rows` rows: tiles of 64 rows, at most one round of workgroup slots (one per CU at hid
// 128, two at 64), and every workgroup the same number of tiles — the launch lasts as long as the workgroup with the most tiles
// either way, and every workgroup fewer is one partial less to sum (PP-hard, E = 8192: 1280 tiles on 256 CUs = 256 workgroups x
// 5, no thin last round).
static int tanh_partials(long long rows, int H, bool wide)
{
    if (rows <= 0 || (H != 64 && H != 128 && !(wide && H == 256))) return 0;
    const long long tiles = (rows + 63) / 64;
    const long long cap = (long long)ic3::device_cus() * (H == 64 ? 2 : 1);
    const long long rounds = (tiles + cap - 1) / cap;
    return (int)((tiles + rounds - 1) / rounds);
}

// both baselines' windows: the tanh kernels' sizes (64 / 128; the _wide entries: 256 too), and the sparse encoder's backward in
// its partial-sums form
static int tanh_supported(const ic3_env* env, int H)
{
    if (!env || (H != 64 && H != 128)) return 0;
    return ic3_bptt_backward_supported(env, H);
}
static int tanh_supported_wide(const ic3_env* env, int H)
{
    if (!env || (H != 64 && H != 128 && H != 256)) return 0;
    return ic3_bptt_backward_supported(env, H);
}
static const char* const TANH_SIZES[2] = { "hid_size 64 / 128", "hid_size 64 / 128 / 256" };
static bool tanh_size_ok(int H, bool wide) { return H == 64 || H == 128 || (wide && H == 256); }

extern "C" int ic3_rnn_backward_partials(long long R, int H) { return tanh_partials(R, H, false); }
extern "C" int ic3_rnn_backward_wide_partials(long long R, int H) { return tanh_partials(R, H, true); }

extern "C" int ic3_rnn_backward_supported(const ic3_env* env, int H) { return tanh_supported(env, H); }
extern "C" int ic3_rnn_backward_wide_supported(const ic3_env* env, int H) { return tanh_supported_wide(env, H); }

extern "C" size_t ic3_rnn_weight_grad_scratch_floats(long long Q, int H)
{
    if (Q <= 0 || (H != 64 && H != 128)) return 0;
    return (size_t)wgrad_plan(Q, 1, 0).ks * H * H;
}
extern "C" size_t ic3_rnn_weight_grad_wide_scratch_floats(long long Q, int H)
{
    if (Q <= 0 || !tanh_size_ok(H, true)) return 0;
    return (size_t)rnn_wgrad_plan(Q, H, H).ks * H * H;
}

// ic3_rnn_weight_grad (hid 64 / 128) and ic3_rnn_weight_grad_wide (64 / 128 / 256) behind their hid_size checks
static int rnn_weight_grad(const float* dz, const float* h_prev, const float* row_live, long long Q, int H, float* dA2, int accumulate,
                           float* scratch, ic3_stream stream, bool wide)
{
    using namespace ic3;
    const char* const fn = wide ? "ic3_rnn_weight_grad_wide: " : "ic3_rnn_weight_grad: ";   // (a std::string only on the way out)
    if (!dz || !h_prev || !dA2 || !scratch || Q <= 0) return fail(-22, std::string(fn) + "null argument");
    if (!tanh_size_ok(H, wide)) return fail(-38, std::string(fn) + TANH_SIZES[wide]);
    const WGradPlan pl = rnn_wgrad_plan(Q, H, H);
    if (!pl.fits) return fail(-22, std::string(fn) + "a K slice must stay below 2 GB (32-bit buffer offsets)");
    const RnnWGradArgs a{ dz, h_prev, row_live, scratch, Q, (int)pl.per };
    hipStream_t s = (hipStream_t)stream;
    // hid 256: the tile of 128 on the four output quadrants (grid y: the dz columns = output rows, z: the h columns)
    const int HT = H == 256 ? 128 : H;
    const size_t lds = (size_t)2 * 2 * 16 * HT * sizeof(float);
    const auto kernel = H == 256 ? rnn_wgrad_kernel<256> : H == 128 ? rnn_wgrad_kernel<128> : rnn_wgrad_kernel<64>;
    const dim3 grid = H == 256 ? dim3(pl.ks, 2, 2) : dim3(pl.ks);
    if (const int rc = launch_kernel(kernel, grid, dim3(256), lds, s, a); rc < 0) return rc;
    return wgrad_reduce(scratch, pl.ks, H * H, dA2, accumulate, s);
}

extern "C" int ic3_rnn_weight_grad(const float* dz, const float* h_prev, const float* row_live, long long Q, int H, float* dA2,
                                   int accumulate, float* scratch, ic3_stream stream)
{
    return rnn_weight_grad(dz, h_prev, row_live, Q, H, dA2, accumulate, scratch, stream, false);
}
extern "C" int ic3_rnn_weight_grad_wide(const float* dz, const float* h_prev, const float* row_live, long long Q, int H, float* dA2,
                                        int accumulate, float* scratch, ic3_stream stream)
{
    return rnn_weight_grad(dz, h_prev, row_live, Q, H, dA2, accumulate, scratch, stream, true);
}

// one step of the chain (also the unit the tests drive): returns the number of partials written / added to
static int rnn_tanh_backward_step(const float* dh_in, const float* h_t, const float* dhead, const float* w_heads, int OT, const float* a2,
                                  const float* out_scale, float* dz, float* dh_out, float* dbias_partials, int accumulate, long long R,
                                  int H, ic3_stream stream, bool wide)
{
    using namespace ic3;
    const char* const fn = wide ? "ic3_rnn_tanh_backward_step_wide: " : "ic3_rnn_tanh_backward_step: ";   // (a std::string only on the way out)
    if (!h_t || !dhead || !w_heads || !a2 || !dz || !dh_out || !dbias_partials || R <= 0) return fail(-22, std::string(fn) + "null argument");
    if (!tanh_size_ok(H, wide)) return fail(-38, std::string(fn) + TANH_SIZES[wide]);
    if (OT < 1 || OT > 16) return fail(-22, std::string(fn) + "1 <= OT <= 16");
    if (R >= (1ll << 31)) return fail(-22, std::string(fn) + "R < 2^31");
    const int grid = tanh_partials(R, H, wide);
    const RnnBwdArgs a{ dh_in, h_t, dhead, w_heads, a2, out_scale, dz, dh_out, dbias_partials, (int)R, OT, (int)((R + 63) / 64),
                        accumulate };
    hipStream_t s = (hipStream_t)stream;
    const int rc = H == 256   ? launch_kernel(rnn_tanh_bwd_kernel<256>, dim3(grid), dim3(1024), TanhTile<256>::LDS_BYTES, s, a)
                   : H == 128 ? launch_kernel(rnn_tanh_bwd_kernel<128>, dim3(grid), dim3(512), TanhTile<128>::LDS_BYTES, s, a)
                              : launch_kernel(rnn_tanh_bwd_kernel<64>, dim3(grid), dim3(256), TanhTile<64>::LDS_BYTES, s, a);
    return rc < 0 ? rc : grid;
}

extern "C" int ic3_rnn_tanh_backward_step(const float* dh_in, const float* h_t, const float* dhead, const float* w_heads, int OT,
                                          const float* a2, const float* out_scale, float* dz, float* dh_out, float* dbias_partials,
                                          int accumulate, long long R, int H, ic3_stream stream)
{
    return rnn_tanh_backward_step(dh_in, h_t, dhead, w_heads, OT, a2, out_scale, dz, dh_out, dbias_partials, accumulate, R, H, stream,
                                  false);
}
extern "C" int ic3_rnn_tanh_backward_step_wide(const float* dh_in, const float* h_t, const float* dhead, const float* w_heads, int OT,
                                               const float* a2, const float* out_scale, float* dz, float* dh_out,
                                               float* dbias_partials, int accumulate, long long R, int H, ic3_stream stream)
{
    return rnn_tanh_backward_step(dh_in, h_t, dhead, w_heads, OT, a2, out_scale, dz, dh_out, dbias_partials, accumulate, R, H, stream,
                                  true);
}

// The window's T steps as ONE launch of rnn_tanh_bwd_walk_kernel (an ic3_rnn_bptt_walk descriptor): the tile plan of the per-step
// launch, one partial row per TILE.
static int rnn_tanh_backward_walk(const ic3_rnn_bptt_walk* b, long long R, ic3_stream stream)
{
    using namespace ic3;
    if (R >= (1ll << 31)) return fail(-22, "ic3_rnn_backward_wide (ic3_rnn_bptt_walk): R < 2^31");
    const int H = b->H, grid = tanh_partials(R, H, true);
    const RnnWalkArgs a{ b->hs, b->h_last, b->dhead, b->w_heads, b->a2, b->row_keep, b->dh, b->dz, b->dbias_partials, (int)R, b->OT,
                         (int)((R + 63) / 64), b->T, b->detach_gap };
    hipStream_t s = (hipStream_t)stream;
    const size_t sums = (size_t)16 * H * sizeof(float);          // the row groups' sums of a step, behind the tile machine's LDS
    return H == 256   ? launch_kernel(rnn_tanh_bwd_walk_kernel<256>, dim3(grid), dim3(1024), TanhTile<256>::LDS_BYTES + sums, s, a)
           : H == 128 ? launch_kernel(rnn_tanh_bwd_walk_kernel<128>, dim3(grid), dim3(512), TanhTile<128>::LDS_BYTES + sums, s, a)
                      : launch_kernel(rnn_tanh_bwd_walk_kernel<64>, dim3(grid), dim3(256), TanhTile<64>::LDS_BYTES + sums, s, a);
}

// B = ic3_rnn_bptt: one launch per step;  B = ic3_rnn_bptt_walk (the _wide entry only): one launch for the T steps — the same checks
// in front, the same encoder stage and weight gradient behind (both read the dz ring and the record only)
template <class B>
static int rnn_backward(ic3_env* env, const B* b, ic3_stream stream, bool wide)
{
    using namespace ic3;
    constexpr bool WALK = std::is_same<B, ic3_rnn_bptt_walk>::value;
    const char* const fn = WALK ? "ic3_rnn_backward_wide (ic3_rnn_bptt_walk)" : wide ? "ic3_rnn_backward_wide" : "ic3_rnn_backward";
    const std::string f = std::string(fn) + ": ";
    if (const int rc = window_open(fn, WALK ? "ic3_rnn_bptt_walk" : "ic3_rnn_bptt", env, b, wide ? tanh_supported_wide : tanh_supported,
                                   (std::string(TANH_SIZES[wide]) + ", a grid whose encoder backward runs in its partial-sums form").c_str(),
                                   false);
        rc < 0)
        return rc;
    const int T = b->T, E = b->E, N = b->N, H = b->H;
    if (!b->hs || !b->dhead || !b->snaps || !b->a2 || !b->w_heads || !b->dh || !b->dz || !b->dbias_partials || !b->enc_work)
        return fail(-22, f + "null argument");
    if (b->a2_grad && !b->wgrad_scratch) return fail(-22, f + "a2_grad needs wgrad_scratch");
    if (b->enc_window && ic3_env_encode_backward_window_work(env, H) <= 0)
        return fail(-22, f + "enc_window on a configuration without ic3_env_encode_backward_window");
    const long long R = (long long)E * N;
    if constexpr (WALK) {
        if (b->reserved) return fail(-22, f + "reserved must be 0");
        if (const int rc = rnn_tanh_backward_walk(b, R, stream); rc < 0) return rc;
        if (const int rc = encoder_tail(env, b->snaps, b->snap_words, T, b->dz, H, R * H, H, b->enc_work, b->enc_first, b->enc_window != 0,
                                        stream);
            rc < 0)
            return rc;
    } else {
        int enc_first = b->enc_first;
        for (int t = T - 1; t >= 0; --t) {
            // trainer.py:56-60: h_t was handed on detached — the launch reads zeros for dL/dh_t (a null input, no memset)
            const bool detached = b->detach_gap > 0 && (t + 1) % b->detach_gap == 0;
            const float* h_t = (t + 1 < T || !b->h_last) ? b->hs + (size_t)(t + 1) * R * H : b->h_last;
            float* dz = b->dz + (size_t)t * R * H;
            int rc = rnn_tanh_backward_step(detached ? nullptr : b->dh, h_t, b->dhead + (size_t)t * R * b->OT, b->w_heads, b->OT, b->a2,
                                            (b->row_keep && t > 0) ? b->row_keep + (size_t)(t - 1) * R : nullptr, dz, b->dh,
                                            b->dbias_partials, 1, R, H, stream, wide);
            if (rc < 0) return rc;
            if (b->enc_window) continue;                         // (the encoder's first stage: once, behind the loop)
            rc = ic3_env_encode_backward_accumulate(env, b->snaps + (size_t)t * b->snap_words, dz, H, H, b->enc_work, enc_first, stream);
            if (rc < 0) return rc;
            enc_first = 0;
        }
        if (b->enc_window) {
            const int rc = ic3_env_encode_backward_window(env, b->snaps, b->snap_words, T, b->dz, H, R * H, H, b->enc_work, enc_first, stream);
            if (rc < 0) return rc;
        }
    }
    if (b->a2_grad) {
        const int rc = rnn_weight_grad(b->dz, b->hs, b->row_live, (long long)T * R, H, b->a2_grad, 1, b->wgrad_scratch, stream, wide);
        if (rc < 0) return rc;
    }
    return 0;
}

extern "C" int ic3_rnn_backward(ic3_env* env, const ic3_rnn_bptt* b, ic3_stream stream) { return rnn_backward(env, b, stream, false); }
extern "C" int ic3_rnn_backward_wide(ic3_env* env, const ic3_rnn_bptt* b, ic3_stream stream)
{
    // (by its second word: a tagged descriptor must have the walk struct's size exactly — window_open refuses it otherwise, before
    //  anything else is read; an untagged one is an ic3_rnn_bptt)
    static_assert(offsetof(ic3_rnn_bptt_walk, magic) == offsetof(ic3_rnn_bptt, T), "the tag sits where ic3_rnn_bptt holds T");
    static_assert(sizeof(ic3_rnn_bptt_walk) != sizeof(ic3_rnn_bptt), "the two descriptors are told apart by their sizes too");
    if (b && (uint32_t)b->T == IC3_RNN_BPTT_WALK_MAGIC) return rnn_backward(env, reinterpret_cast<const ic3_rnn_bptt_walk*>(b), stream, true);
    return rnn_backward(env, b, stream, true);
}

// ---------------------------------------------------------------------------------------------------------------------------
// ic3_mlp_backward: the IC baseline (models.py:23-34, models.MLP), every step on its own:
//     e = affine1(obs),   x1 = tanh(e),   h = tanh(affine2(x1) + x1),   [logits | value] = W_heads h + b
// differentiated over a window of recorded steps.  No state crosses a step, so the window is Q = T x R independent rows and the
// backward is ONE launch over all of them (mlp_bwd_kernel):
//     x1  = tanh(e)                                        -> over e (the ring slot holds x1 afterwards)
//     dz  = (d . W_heads) (1 - h^2)                        -> the dz ring (affine2's pre-activation gradient)
//     de  = (dz . A2 + dz) (1 - x1^2)                      -> the de ring (affine1's; the `+ dz` is the skip)
//     per-workgroup column sums of dz                      (d affine2.bias; fixed-order reduction by the caller)
// behind it the encoder's first stage over the de ring and ONE rnn_wgrad_kernel launch for dA2 += dz^T . x1 over all Q rows.
//
// mlp_bwd_kernel<H>: the shape of rnn_tanh_bwd_kernel — 4H threads, persistent over tiles of 64 rows, A2 in LDS in fragment order
// for the workgroup's life.  Per tile: phase 0 — thread (row group, 4-column chunk) forms x1 and dz for 4 rows, stores both with
// 16-byte stores, dz also to the LDS tile and into its column sums; phase 1 — wave (rb, cb) multiplies tile rows [32 rb, +32) by
// A2's columns [32 cb, +32); epilogue — the accumulators go back through the LDS tile (over the dz rows every wave is done with)
// and thread (row group, chunk) combines them with the dz / x1 it still holds and stores de 16 bytes per lane (4-byte stores from
// the accumulator layout cost 1.3 x the write traffic in lstm_gates_bwd_kernel).  The next tile's rows are requested before the
// product, so the matrix phase of a tile covers the loads of the next.  Row offsets in 64 bits (TJ-hard: 13.1 M rows x 512 B).
// LDS as rnn_tanh_bwd_kernel (110 KB at H = 128: one workgroup of 8 waves per CU; 41 KB at 64: two of 4; 85 KB at 256, where A2's
// fragments are streamed from L2: the plan in the block above rnn_tanh_bwd_kernel).
// HBM per row: e, h in, x1, dz, de out (5 H floats) + OT; MFMA 2 H^2 flop per row on the fp32 instruction.
// ---------------------------------------------------------------------------------------------------------------------------
namespace ic3 {

struct MlpBwdArgs {
    float* x1;               // [Q][H] in: e, out: x1 = tanh(e)
    const float* h;          // [Q][H]
    const float* dhead;      // [Q][OT]
    const float* w_heads;    // [OT][H]
    const float* a2;         // [H][H] affine2.weight (out, in): d x1 = dz . A2 + dz
    float* dz;               // [Q][H]
    float* de;               // [Q][H]
    float* db_part;          // [gridDim.x][H]
    long long Q;
    int OT, tiles, accumulate;
};

template <int H>
__global__ __launch_bounds__(4 * H, (H <= 64) ? 2 : 1) void mlp_bwd_kernel(const MlpBwdArgs a)
{
    using Tile = TanhTile<H>;
    constexpr int NT = Tile::NT, LDA = Tile::LDA, LDA4 = Tile::LDA4, RPP = Tile::RPP, PER = Tile::PER;
    constexpr int DPT = 64 * 16 / NT;                            // d values a thread stages per tile, at most
    static_assert(DPT * NT == 64 * 16, "tile split");
    IC3_DYNAMIC_LDS(float, smem);
    const Tile t(smem);                                          // (Dz: the tile's dz, then its dz . A2)
    const int OT = a.OT;
    t.stage_weights(a.a2, a.w_heads, OT);
    bp_f32x4 bsum = { 0.f, 0.f, 0.f, 0.f };
    bp_f32x4 ev[PER], hv[PER];
    float dp[DPT];
    // (rows past the window read 0 and their stores are dropped: the ranges of the buffer descriptors)
    auto fetch = [&](int tile) {
        const long long r0 = (long long)tile * 64;
        const int rows = (a.Q - r0) < 64 ? (int)(a.Q - r0) : 64;
        const __amdgpu_buffer_rsrc_t re = bp_rsrc(a.x1 + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rh = bp_rsrc(a.h + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rd = bp_rsrc(a.dhead + r0 * OT, (long long)rows * OT * 4);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int off = ((t.rg + RPP * i) * H + 4 * t.c4) * 4;
            ev[i] = bp_load4(re, off);
            hv[i] = bp_load4(rh, off);
        }
#pragma unroll
        for (int i = 0; i < DPT; ++i) dp[i] = bp_load1(rd, (t.tid + i * NT) * 4);    // (past 64 OT: past the range, 0)
    };
    if ((int)blockIdx.x < a.tiles) fetch(blockIdx.x);
    __syncthreads();
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * 64;
        const int rows = (a.Q - r0) < 64 ? (int)(a.Q - r0) : 64;
        const __amdgpu_buffer_rsrc_t rx = bp_rsrc(a.x1 + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rz = bp_rsrc(a.dz + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rde = bp_rsrc(a.de + r0 * H, (long long)rows * H * 4);
#pragma unroll
        for (int i = 0; i < DPT; ++i) t.Sd[t.tid + i * NT] = dp[i];
        __syncthreads();
        // ---- phase 0: x1 over e; dz of the tile -> ring, LDS, column sums
        bp_f32x4 xv[PER], zv[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int row = t.rg + RPP * i;
            bp_f32x4 x;
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = fast_tanh(ev[i][q]);
            const bp_f32x4 v = t.heads_share(bp_f32x4{ 0.f, 0.f, 0.f, 0.f }, row, OT);
            const bp_f32x4 z = v * (1.0f - hv[i] * hv[i]);
            bsum += z;
            xv[i] = x;
            zv[i] = z;
            t.Dz4[row * LDA4 + t.c4] = z;
            bp_store4(x, rx, (row * H + 4 * t.c4) * 4);
            bp_store4(z, rz, (row * H + 4 * t.c4) * 4);
        }
        if (tile + (int)gridDim.x < a.tiles) fetch(tile + gridDim.x);       // the next tile's rows, in flight under the product
        __syncthreads();
        // ---- phase 1: dz . A2
        const bp_f32x16 acc = t.product(a.a2);
        __syncthreads();                                         // every wave has read the tile's dz rows
        // ---- epilogue: the product back through the LDS tile, de = (dz . A2 + dz)(1 - x1^2) in the phase-0 layout
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            t.Dz[(32 * t.rb + (reg & 3) + 8 * (reg >> 2) + 4 * t.lh) * LDA + 32 * t.cb + t.li] = acc[reg];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int row = t.rg + RPP * i;
            const bp_f32x4 g = (t.Dz4[row * LDA4 + t.c4] + zv[i]) * (1.0f - xv[i] * xv[i]);
            bp_store4(g, rde, (row * H + 4 * t.c4) * 4);
        }
        __syncthreads();                                         // every thread is done with the tile's LDS
    }
    t.column_sums(bsum, a.db_part, a.accumulate);
}

}  // namespace ic3

// Tile plan of the launch: as ic3_rnn_backward_partials, over the Q rows of the window (one launch, not one per step).
extern "C" int ic3_mlp_backward_partials(long long Q, int H) { return tanh_partials(Q, H, false); }
extern "C" int ic3_mlp_backward_wide_partials(long long Q, int H) { return tanh_partials(Q, H, true); }

extern "C" int ic3_mlp_backward_supported(const ic3_env* env, int H) { return tanh_supported(env, H); }
extern "C" int ic3_mlp_backward_wide_supported(const ic3_env* env, int H) { return tanh_supported_wide(env, H); }

// the launch alone (also the unit the tests drive): returns the number of partials written / added to
static int mlp_backward_step(float* x1_inout, const float* h, const float* dhead, const float* w_heads, int OT, const float* a2, float* dz,
                             float* de, float* dbias_partials, int accumulate, long long Q, int H, ic3_stream stream, bool wide)
{
    using namespace ic3;
    const char* const fn = wide ? "ic3_mlp_backward_step_wide: " : "ic3_mlp_backward_step: ";   // (a std::string only on the way out)
    if (!x1_inout || !h || !dhead || !w_heads || !a2 || !dz || !de || !dbias_partials || Q <= 0) return fail(-22, std::string(fn) + "null argument");
    if (!tanh_size_ok(H, wide)) return fail(-38, std::string(fn) + TANH_SIZES[wide]);
    if (OT < 1) return fail(-22, std::string(fn) + "OT >= 1");
    if (OT > 16) return fail(-38, std::string(fn) + "at most 16 output columns");
    if (Q >= (1ll << 36)) return fail(-22, std::string(fn) + "Q < 2^36");
    const int grid = tanh_partials(Q, H, wide);
    const MlpBwdArgs a{ x1_inout, h, dhead, w_heads, a2, dz, de, dbias_partials, Q, OT, (int)((Q + 63) / 64), accumulate };
    hipStream_t s = (hipStream_t)stream;
    const int rc = H == 256   ? launch_kernel(mlp_bwd_kernel<256>, dim3(grid), dim3(1024), TanhTile<256>::LDS_BYTES, s, a)
                   : H == 128 ? launch_kernel(mlp_bwd_kernel<128>, dim3(grid), dim3(512), TanhTile<128>::LDS_BYTES, s, a)
                              : launch_kernel(mlp_bwd_kernel<64>, dim3(grid), dim3(256), TanhTile<64>::LDS_BYTES, s, a);
    return rc < 0 ? rc : grid;
}

extern "C" int ic3_mlp_backward_step(float* x1_inout, const float* h, const float* dhead, const float* w_heads, int OT, const float* a2,
                                     float* dz, float* de, float* dbias_partials, int accumulate, long long Q, int H,
                                     ic3_stream stream)
{
    return mlp_backward_step(x1_inout, h, dhead, w_heads, OT, a2, dz, de, dbias_partials, accumulate, Q, H, stream, false);
}
extern "C" int ic3_mlp_backward_step_wide(float* x1_inout, const float* h, const float* dhead, const float* w_heads, int OT,
                                          const float* a2, float* dz, float* de, float* dbias_partials, int accumulate, long long Q,
                                          int H, ic3_stream stream)
{
    return mlp_backward_step(x1_inout, h, dhead, w_heads, OT, a2, dz, de, dbias_partials, accumulate, Q, H, stream, true);
}

static int mlp_backward(ic3_env* env, const ic3_mlp_bptt* b, ic3_stream stream, bool wide)
{
    using namespace ic3;
    const char* const fn = wide ? "ic3_mlp_backward_wide" : "ic3_mlp_backward";
    const std::string f = std::string(fn) + ": ";
    if (int rc = window_open(fn, "ic3_mlp_bptt", env, b, wide ? tanh_supported_wide : tanh_supported,
                             (std::string(TANH_SIZES[wide]) + ", a grid whose encoder backward runs in its partial-sums form").c_str(),
                             true);
        rc < 0)
        return rc;
    const int T = b->T, E = b->E, N = b->N, H = b->H;
    if (!b->h || !b->dhead || !b->snaps || !b->enc_wt || !b->enc_bias || !b->a2 || !b->w_heads || !b->x1 || !b->dz || !b->de ||
        !b->dbias_partials || !b->enc_work)
        return fail(-22, f + "null argument");
    if (b->a2_grad && !b->wgrad_scratch) return fail(-22, f + "a2_grad needs wgrad_scratch");
    if (b->enc_window && ic3_env_encode_backward_window_work(env, H) <= 0)
        return fail(-22, f + "enc_window on a configuration without ic3_env_encode_backward_window");
    const long long R = (long long)E * N, Q = (long long)T * R;
    // e of every recorded step -> the slots of the x1 ring (the step launch does not record its encoder rows)
    for (int t = 0; t < T; ++t) {
        const int rc = ic3_env_encode_at(env, b->snaps + (size_t)t * b->snap_words, b->enc_wt, b->enc_bias, b->loc_table,
                                         b->x1 + (size_t)t * R * H, H, H, stream);
        if (rc < 0) return rc;
    }
    int rc = mlp_backward_step(b->x1, b->h, b->dhead, b->w_heads, b->OT, b->a2, b->dz, b->de, b->dbias_partials, 0, Q, H, stream, wide);
    if (rc < 0) return rc;
    rc = encoder_tail(env, b->snaps, b->snap_words, T, b->de, H, R * H, H, b->enc_work, b->enc_first, b->enc_window != 0, stream);
    if (rc < 0) return rc;
    if (b->a2_grad) {
        rc = rnn_weight_grad(b->dz, b->x1, nullptr, Q, H, b->a2_grad, 1, b->wgrad_scratch, stream, wide);
        if (rc < 0) return rc;
    }
    return 0;
}

extern "C" int ic3_mlp_backward(ic3_env* env, const ic3_mlp_bptt* b, ic3_stream stream) { return mlp_backward(env, b, stream, false); }
extern "C" int ic3_mlp_backward_wide(ic3_env* env, const ic3_mlp_bptt* b, ic3_stream stream) { return mlp_backward(env, b, stream, true); }

// ---------------------------------------------------------------------------------------------------------------------------
// ic3_commnet_backward: the NON-recurrent CommNet module (comm.py:127-129, 179-224; the forward of commnet_fwd.hip),
//     x = h_0 = tanh(enc),   h_{i+1} = tanh(x + F_i h_i + C_i mix(h_i) + b_i)   i = 0 .. P - 1,   [logits | value] = W_heads h_P + b
// differentiated over a window of recorded steps.  No state crosses a step: the window is Q = T x R independent rows in T x E
// independent envs, and the backward is a chain of window-wide launches — every one of them a launch the library already had,
// but for the two small kernels below:
//     T x ic3_env_encode_at                       enc of every snapshot -> slot 0 of the h_pass ring
//     ic3_commnet_forward_record over T x E envs  h_0 .. h_P of every row -> the ring (slot 0 over enc: a workgroup owns its rows)
//     per pass i = P - 1 .. 0:
//       commnet_pass_bwd_kernel                   dz_i = (dh_{i+1} [+ d . W_heads: last pass]) (1 - h_{i+1}^2) -> [dz_i | dz_i F_i] rows,
//                                                 the dz slot, dx (+)= dz_i, column sums of dz_i (d b_i) as per-workgroup partials
//       ic3_comm_backward on [dz_i | dz_i F_i]    dh_i = dz_i F_i + mix(dz_i) C_i,  dC_i partials = mix(dz_i)^T h_i   (the mixing matrix
//                                                 is symmetric: mix(dz C) = mix(dz) C and dz^T mix(h) = mix(dz)^T h)
//       ic3_rnn_weight_grad_wide                  dF_i += dz_i^T h_i over all rows
//       wgrad_reduce x 2                          dC_i += its partials, d b_i += its partials, in partial order
//     commnet_de_kernel                           de = (dx + dh_0)(1 - h_0^2)
//     encoder_tail                                the sparse encoder's stage 1 over the de ring
//     ic3_heads_grad                              (with heads_w_grad) the heads' gradient on slot P of the ring
// all on the caller's stream.
//
// commnet_pass_bwd_kernel<H>: the tile machine of rnn_tanh_bwd_kernel (TanhTile<H>: 4H threads, persistent over 64-row tiles, F_i in
// LDS in fragment order at 64 / 128, its fragments streamed from L2 at 256, buffer descriptors whose ranges drop the rows past the
// window) with mlp_bwd_kernel's epilogue (the product back through the LDS tile, 16-byte stores) and 64-bit row offsets.  dz is
// stored TWICE — columns [0, H) of the [Q][2H] rows ic3_comm_backward reads and the contiguous [Q][H] slot the weight gradient
// reads (rnn_wgrad_kernel has no leading dimension) — H floats = 4 H bytes per row and pass more than a fused chain would move
// (512 B at H = 128): accepted here, the stages are launches the library already tests.
// HBM per row and pass: dh_in, h_{i+1}, dx in, dz twice, dz F_i, dx out = 7 H floats (+ OT on the last pass); MFMA 2 H^2 flop.
// ---------------------------------------------------------------------------------------------------------------------------
namespace ic3 {

struct CommnetPassArgs {
    const float* dh_in;      // [Q][H] or null (zeros)
    const float* h_next;     // [Q][H] h_{i+1}
    const float* dhead;      // [Q][OT] or null (OT == 0 then)
    const float* w_heads;    // [OT][H]
    const float* fw;         // [H][H] f_modules[i].weight (out, in): dz . F_i
    float* dxh;              // [Q][2H]: [dz | dz . F_i]
    float* dz;               // [Q][H]
    float* dx;               // [Q][H]: = dz (dx_add == 0) or += dz
    float* db_part;          // [gridDim.x][H]
    long long Q;
    int OT, tiles, dx_add, accumulate;
};

template <int H>
__global__ __launch_bounds__(4 * H, (H <= 64) ? 2 : 1) void commnet_pass_bwd_kernel(const CommnetPassArgs a)
{
    using Tile = TanhTile<H>;
    constexpr int NT = Tile::NT, LDA = Tile::LDA, LDA4 = Tile::LDA4, RPP = Tile::RPP, PER = Tile::PER;
    IC3_DYNAMIC_LDS(float, smem);
    const Tile t(smem);                                          // (Dz: the tile's dz, then its dz . F_i)
    const int OT = a.OT;
    t.stage_weights(a.fw, a.w_heads, OT);
    bp_f32x4 bsum = { 0.f, 0.f, 0.f, 0.f };
    __syncthreads();
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * 64;
        const int rows = (a.Q - r0) < 64 ? (int)(a.Q - r0) : 64;
        // (rows past the window read 0 and their stores are dropped: the ranges of the buffer descriptors)
        const __amdgpu_buffer_rsrc_t rdi = bp_rsrc(a.dh_in ? a.dh_in + r0 * H : a.h_next, a.dh_in ? (long long)rows * H * 4 : 0);
        const __amdgpu_buffer_rsrc_t rh = bp_rsrc(a.h_next + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rd = bp_rsrc(a.dhead ? a.dhead + r0 * OT : a.h_next, a.dhead ? (long long)rows * OT * 4 : 0);
        const __amdgpu_buffer_rsrc_t rz = bp_rsrc(a.dz + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rx = bp_rsrc(a.dx + r0 * H, (long long)rows * H * 4);
        const __amdgpu_buffer_rsrc_t rxh = bp_rsrc(a.dxh + r0 * 2 * H, (long long)rows * 2 * H * 4);
        bp_f32x4 dv[PER], hv[PER], xv[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int off = ((t.rg + RPP * i) * H + 4 * t.c4) * 4;
            dv[i] = bp_load4(rdi, off);
            hv[i] = bp_load4(rh, off);
            xv[i] = a.dx_add ? bp_load4(rx, off) : bp_f32x4{ 0.f, 0.f, 0.f, 0.f };
        }
        for (int i = t.tid; i < 64 * OT; i += NT) t.Sd[i] = bp_load1(rd, i * 4);
        __syncthreads();
        // ---- phase 0: dz of the tile -> the [dz | .] rows, the dz slot, dx, LDS, column sums
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int row = t.rg + RPP * i;
            const bp_f32x4 v = t.heads_share(dv[i], row, OT);
            const bp_f32x4 z = v * (1.0f - hv[i] * hv[i]);
            bsum += z;
            t.Dz4[row * LDA4 + t.c4] = z;
            bp_store4(z, rz, (row * H + 4 * t.c4) * 4);
            bp_store4(z, rxh, (row * 2 * H + 4 * t.c4) * 4);
            bp_store4(xv[i] + z, rx, (row * H + 4 * t.c4) * 4);
        }
        __syncthreads();
        // ---- phase 1: dz . F_i
        const bp_f32x16 acc = t.product(a.fw);
        __syncthreads();                                         // every wave has read the tile's dz rows
        // ---- epilogue: the product back through the LDS tile, stored 16 bytes per lane into columns [H, 2H)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            t.Dz[(32 * t.rb + (reg & 3) + 8 * (reg >> 2) + 4 * t.lh) * LDA + 32 * t.cb + t.li] = acc[reg];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int row = t.rg + RPP * i;
            bp_store4(t.Dz4[row * LDA4 + t.c4], rxh, (row * 2 * H + H + 4 * t.c4) * 4);
        }
        __syncthreads();                                         // every thread is done with the tile's LDS
    }
    t.column_sums(bsum, a.db_part, a.accumulate);
}

// de = (dx + dh_0)(1 - h_0^2) over Q rows of H floats (n4 float4): through x = h_0 = tanh(enc)
__global__ __launch_bounds__(256) void commnet_de_kernel(const bp_f32x4* __restrict__ dx, const bp_f32x4* __restrict__ dh0,
                                                         const bp_f32x4* __restrict__ h0, bp_f32x4* __restrict__ de, long long n4)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const bp_f32x4 x = h0[i];
        de[i] = (dx[i] + dh0[i]) * (1.0f - x * x);
    }
}

}  // namespace ic3

extern "C" int ic3_commnet_backward_supported(const ic3_env* env, int H, int N)
{
    if (!env || N != env->dims.N || !ic3_commnet_forward_supported(H, N)) return 0;
    return tanh_supported_wide(env, H);
}

extern "C" int ic3_commnet_pass_backward_partials(long long Q, int H) { return tanh_partials(Q, H, true); }

// the pass launch alone (also the unit the tests drive): returns the number of partials written / added to
extern "C" int ic3_commnet_pass_backward(const float* dh_in, const float* h_next, const float* dhead, const float* w_heads, int OT,
                                         const float* f_weight, float* dxh, float* dz, float* dx, int dx_add, float* dbias_partials,
                                         int accumulate, long long Q, int H, ic3_stream stream)
{
    using namespace ic3;
    const char* const fn = "ic3_commnet_pass_backward: ";
    if (!h_next || !f_weight || !dxh || !dz || !dx || !dbias_partials || Q <= 0 || (dhead && !w_heads))
        return fail(-22, std::string(fn) + "null argument");
    if (!tanh_size_ok(H, true)) return fail(-38, std::string(fn) + TANH_SIZES[1]);
    if (!dhead) OT = 0;
    else if (OT < 1) return fail(-22, std::string(fn) + "OT >= 1");
    else if (OT > 16) return fail(-38, std::string(fn) + "at most 16 output columns");
    if (Q >= (1ll << 36)) return fail(-22, std::string(fn) + "Q < 2^36");
    const int grid = tanh_partials(Q, H, true);
    const CommnetPassArgs a{ dh_in, h_next, dhead, w_heads, f_weight, dxh, dz, dx, dbias_partials, Q, OT, (int)((Q + 63) / 64),
                             dx_add, accumulate };
    hipStream_t s = (hipStream_t)stream;
    const int rc = H == 256   ? launch_kernel(commnet_pass_bwd_kernel<256>, dim3(grid), dim3(1024), TanhTile<256>::LDS_BYTES, s, a)
                   : H == 128 ? launch_kernel(commnet_pass_bwd_kernel<128>, dim3(grid), dim3(512), TanhTile<128>::LDS_BYTES, s, a)
                              : launch_kernel(commnet_pass_bwd_kernel<64>, dim3(grid), dim3(256), TanhTile<64>::LDS_BYTES, s, a);
    return rc < 0 ? rc : grid;
}

// The steps of one chunk of a window: as many as keep every launch of the chain inside its 32-bit limits — the envs of a chunk as
// one int (ic3_comm_backward, the forward: T' x E), its rows below 2^31 - 2^16 (the encoder's window form), the weight gradient's K
// slices below 2 GB (rnn_wgrad_plan) — and at most `most` (> 0: the caller's bound).
static int commnet_chunk_steps(int T, int E, int N, int H, int most)
{
    const long long R = (long long)E * N;
    long long tc = std::min<long long>(T, ((1ll << 31) - (1ll << 16)) / R);
    if (most > 0) tc = std::min<long long>(tc, most);
    while (tc > 1 && !rnn_wgrad_plan(tc * R, H, H).fits) tc = (tc + 1) / 2;
    return tc < 1 ? 0 : (int)tc;
}

extern "C" int ic3_commnet_backward_chunk_steps(const ic3_env* env, int T, int H, int max_chunk_steps)
{
    if (!env || T <= 0 || !tanh_size_ok(H, true)) return 0;
    return commnet_chunk_steps(T, env->dims.E, env->dims.N, H, max_chunk_steps);
}

// scratch of a window run in chunks of Tc steps, in floats: [bias partials | dC partials | weight-gradient slices | heads] — each
// the larger of what a full chunk and the short last one ask for (a larger launch may leave FEWER partials: more rounds)
struct CommnetScratch {
    size_t bias, dcw, wgrad, heads;
    size_t total() const { return bias + dcw + wgrad + heads; }
};
static CommnetScratch commnet_scratch(int T, int Tc, int E, int N, int H)
{
    CommnetScratch sc{ 0, 0, 0, ic3_heads_grad_scratch_floats(H) };
    for (const int tn : { Tc, T % Tc }) {
        if (!tn) continue;
        const long long Q = (long long)tn * E * N;
        sc.bias = std::max(sc.bias, (size_t)tanh_partials(Q, H, true) * H);
        sc.dcw = std::max(sc.dcw, (size_t)ic3_comm_backward_partials(tn * E, N) * H * H);
        sc.wgrad = std::max(sc.wgrad, ic3_rnn_weight_grad_wide_scratch_floats(Q, H));
    }
    return sc;
}

extern "C" size_t ic3_commnet_backward_scratch_floats(const ic3_env* env, int T, int H, int max_chunk_steps)
{
    const int tc = ic3_commnet_backward_chunk_steps(env, T, H, max_chunk_steps);
    if (!tc) return 0;
    return commnet_scratch(T, tc, env->dims.E, env->dims.N, H).total();
}

extern "C" int ic3_commnet_backward(ic3_env* env, const ic3_commnet_bptt* b, ic3_stream stream)
{
    using namespace ic3;
    const char* const fn = "ic3_commnet_backward";
    const std::string f = std::string(fn) + ": ";
    if (const int rc = window_open(fn, "ic3_commnet_bptt", env, b, tanh_supported_wide,
                                   "hid_size 64 / 128 / 256, a grid whose encoder backward runs in its partial-sums form", true);
        rc < 0)
        return rc;
    const int T = b->T, E = b->E, N = b->N, H = b->H, P = b->passes, OT = b->OT;
    if (N > 64) return fail(-38, f + "at most 64 agents per env");
    if (P < 1 || b->max_chunk_steps < 0) return fail(-22, f + "passes >= 1, max_chunk_steps >= 0");
    if (!b->dhead || !b->snaps || !b->enc_wt || !b->enc_bias || !b->wp || !b->bias || !b->w_heads || !b->f_weight || !b->f_grad ||
        !b->bias_grad || !b->h_pass || !b->dxh || !b->dz || !b->dx || !b->de || !b->dh || !b->scratch || !b->enc_work)
        return fail(-22, f + "null argument");
    if (!b->comm_zero && (!b->c_weight || !b->c_grad)) return fail(-22, f + "C's weights and their gradients");
    if ((b->heads_w_grad != nullptr) != (b->heads_b_grad != nullptr)) return fail(-22, f + "heads_w_grad and heads_b_grad come together");
    for (int i = 0; i < P; ++i)
        if (!b->f_weight[i] || !b->f_grad[i] || !b->bias_grad[i] || (!b->comm_zero && (!b->c_weight[i] || !b->c_grad[i])))
            return fail(-22, f + "null per-pass pointer");
    if (b->enc_window && ic3_env_encode_backward_window_work(env, H) <= 0)
        return fail(-22, f + "enc_window on a configuration without ic3_env_encode_backward_window");
    const int Tc = commnet_chunk_steps(T, E, N, H, b->max_chunk_steps);
    if (!Tc) return fail(-22, f + "one step of the window is past the launches' 32-bit limits");
    const long long R = (long long)E * N;
    const CommnetScratch sc = commnet_scratch(T, Tc, E, N, H);
    float* const bias_parts = b->scratch;
    float* const dcw_parts = bias_parts + sc.bias;
    float* const wg_scratch = dcw_parts + sc.dcw;
    float* const heads_scratch = wg_scratch + sc.wgrad;
    hipStream_t s = (hipStream_t)stream;
    int enc_first = b->enc_first;
    for (int t0 = 0; t0 < T; t0 += Tc) {
        const int tn = std::min(Tc, T - t0);
        const long long Q = (long long)tn * R;
        const size_t ring = (size_t)Q * H;                        // floats between two slots of the h_pass ring: this chunk's rows
        const int32_t* snaps = b->snaps + (size_t)t0 * b->snap_words;
        const int32_t* alive = b->alive ? b->alive + (size_t)t0 * R : nullptr;
        const int32_t* gate = b->gate ? b->gate + (size_t)t0 * R : nullptr;
        const float* dhead = b->dhead + (size_t)t0 * R * OT;
        // 1. enc of every recorded step -> slot 0 of the ring
        for (int t = 0; t < tn; ++t) {
            const int rc = ic3_env_encode_at(env, snaps + (size_t)t * b->snap_words, b->enc_wt, b->enc_bias, b->loc_table,
                                             b->h_pass + (size_t)t * R * H, H, H, stream);
            if (rc < 0) return rc;
        }
        // 2. the forward again, h_0 .. h_P kept (h_0 over enc)
        int rc = ic3_commnet_forward_record(b->h_pass, tn * E, N, H, P, b->wp, b->wp3, b->bias, nullptr, nullptr, nullptr, 0, b->mode_avg,
                                            b->comm_zero, alive, gate, nullptr, nullptr, b->h_pass, stream);
        if (rc < 0) return rc;
        // 3. the passes, last to first
        for (int i = P - 1; i >= 0; --i) {
            const bool last = i == P - 1;
            rc = ic3_commnet_pass_backward(last ? nullptr : b->dh, b->h_pass + (size_t)(i + 1) * ring, last ? dhead : nullptr, b->w_heads, OT,
                                           b->f_weight[i], b->dxh, b->dz, b->dx, last ? 0 : 1, bias_parts, 0, Q, H, stream);
            if (rc < 0) return rc;
            const int nb = rc;
            rc = ic3_comm_backward(b->dxh, 2 * H, b->h_pass + (size_t)i * ring, alive, gate, b->comm_zero ? nullptr : b->c_weight[i], nullptr,
                                   b->dh, dcw_parts, 0, tn * E, N, H, b->mode_avg, b->comm_zero, stream);
            if (rc < 0) return rc;
            const int nc = rc;
            rc = rnn_weight_grad(b->dz, b->h_pass + (size_t)i * ring, nullptr, Q, H, b->f_grad[i], 1, wg_scratch, stream, true);
            if (rc < 0) return rc;
            if (nc > 0 && (rc = wgrad_reduce(dcw_parts, nc, H * H, b->c_grad[i], 1, s)) < 0) return rc;
            if ((rc = wgrad_reduce(bias_parts, nb, H, b->bias_grad[i], 1, s)) < 0) return rc;
        }
        // 4. through x = h_0 = tanh(enc)
        {
            const long long n4 = Q * (H / 4);
            const int blocks = (int)std::min<long long>((n4 + 255) / 256, 4096);
            rc = launch_kernel(commnet_de_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const bp_f32x4*>(b->dx),
                               reinterpret_cast<const bp_f32x4*>(b->dh), reinterpret_cast<const bp_f32x4*>(b->h_pass),
                               reinterpret_cast<bp_f32x4*>(b->de), n4);
            if (rc < 0) return rc;
        }
        // 5. the sparse encoder's stage 1 over the de ring
        rc = encoder_tail(env, snaps, b->snap_words, tn, b->de, H, R * H, H, b->enc_work, enc_first, b->enc_window != 0, stream);
        if (rc < 0) return rc;
        enc_first = 0;
        // 6. the heads' gradient on h_P
        if (b->heads_w_grad) {
            rc = ic3_heads_grad(dhead, b->h_pass + (size_t)P * ring, Q, H, OT, b->heads_w_grad, b->heads_b_grad, heads_scratch, stream);
            if (rc < 0) return rc;
        }
    }
    return (T + Tc - 1) / Tc;     // chunks run
}
