// step_launch.hpp — the host side of what the two one-launch rollout steps share (ic3_policy_step in policy_step.hip,
// ic3_commnet_step in commnet_fwd.hip, and their forward-only siblings): the size of a tile's env-descriptor block in LDS, the env
// half of the kernels' argument blocks, the hid_size dispatch and the launch that stamps the caller's two events.
#pragma once
#include <hip/hip_ext.h>

#include <type_traits>

#include "env_device.hpp"
#include "ic3_common.hpp"

namespace ic3 {

// int32 words of the env-descriptor block of one tile (EPT = 64 / N whole envs) in LDS.  The kernels index LDS by it, so it
// mirrors the device-side layout the kernels build there (env_device.hpp):
//   PP: sr[EPT * total] | sc[EPT * total] (rounded up to 4 words) | tab[EPT * N * WW] (int2), total = predators + prey;
//   TJ: EPT blocks of tj_tile_words(N, WW) = [sr | sc | sal | s0 .. s3] (7 N words, rounded up to 4) | tab[N * WW] (int2).
inline size_t step_tile_words(const ic3_env* env)
{
    const int N = env->dims.N, EPT = 64 / N, WW = env->dims.window * env->dims.window;
    size_t w;
    if (env->kind == IC3_ENV_PP) w = (size_t)((2 * EPT * (env->pp.N + env->pp.nprey) + 3) & ~3) + (size_t)2 * EPT * N * WW;
    else w = (size_t)EPT * (((7 * N + 3) & ~3) + 2 * N * WW);
    return (w + 3) & ~(size_t)3;
}

// The env half of StepArgs / CommnetArgs (the same field names in both) from the handle: tile geometry, Philox key, the state's
// device views, where env.step reports.  `take_events`: this is the step's LAST launch — the one-shot events armed by
// ic3_env_set_step_events are handed to it (and disarmed), otherwise they stay armed.
template <class Args>
inline void fill_env_args(Args& a, ic3_env* env, float* reward, int32_t* done, int32_t* alive, int32_t* is_completed,
                          bool take_events, hipEvent_t& ev0, hipEvent_t& ev1)
{
    a.E = env->dims.E;
    a.N = env->dims.N;
    a.EPT = 64 / a.N;
    a.episode = env->f("episode");
    a.tstep = env->f("t");
    a.so = StepOut{ reward, done, alive, is_completed, env->d_err };
    if (env->kind == IC3_ENV_PP) {
        a.pp = pp_state_of(env);
        a.G = group_lanes(a.N);
        a.seed = env->pp.seed;
        a.gid0 = env->pp.env_id_offset;
    } else {
        a.tj = tj_state_of(env);
        a.G = tj_group(a.N);
        a.seed = env->tj.seed;
        a.gid0 = env->tj.env_id_offset;
    }
    a.tile_words = (int)step_tile_words(env);
    a.obs_dim = env->dims.obs_dim;
    a.auto_reset = env->auto_max_steps > 0;
    ev0 = ev1 = nullptr;
    if (take_events) {
        ev0 = (hipEvent_t)env->ev_start;
        ev1 = (hipEvent_t)env->ev_stop;
        env->ev_start = env->ev_stop = nullptr;
    }
}

// ic3_policy_step on an ic3_commnet_window (commnet_fwd.hip): ic3_policy_step's arguments behind the descriptor's tag and size check
// (`wide`: the tag was IC3_COMMNET_WINDOW_WIDE)
int commnet_step_window(ic3_env* env, const ic3_commnet_window* w, bool wide, float* h, float* c, const int32_t* alive_in, const int32_t* comm_in,
                        float* out, int32_t* action, float* obs, float* reward, int32_t* done, int32_t* alive, int32_t* is_completed,
                        ic3_stream stream);

// f(std::integral_constant<int, H>) for hid_size 64 / 128 / 256 (every caller has refused any other H before it plans a launch).
// What f instantiates is what gets built: an instantiation that exists for some H only stays outside (policy_step.hip's pass loop).
template <class F>
inline int with_hid(int H, F&& f)
{
    if (H == 64) return f(std::integral_constant<int, 64>{});
    if (H == 128) return f(std::integral_constant<int, 128>{});
    return f(std::integral_constant<int, 256>{});
}

// launch_kernel (ic3_common.hpp) with the dispatch itself stamping the two events (no separate record packets around it)
template <class... P, class... A>
inline int launch_kernel_timed(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t ev0,
                               hipEvent_t ev1, const A&... args)
{
    if (lds) IC3_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds));
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, ev0, ev1, 0, args...);
    IC3_HIP(hipGetLastError());
    return 0;
}

}  // namespace ic3
