// dispatch.h — the kernel table: one Entry per model, one Kernel per (method, trajectory,
// store policy, ...) slot, one launch() for all of them.  A built-in model's slots hold the
// addresses of its kernels, instantiated in its own translation unit (inst_*.hip) so the
// library builds in parallel; a run-time compiled model's slots hold the functions of its
// hipRTC module (rtc.hip).  A null slot: the model does not have that kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "ode_kernels.cuh"

namespace oe {

// widest model with the producer/consumer RK4 trajectory kernels
#ifndef OE_PIPE_MAX_S
#define OE_PIPE_MAX_S 32  // every built-in (A/B: the piped XCD-ordered kernels win up to chain20)
#endif

// ---- dispatch table ---------------------------------------------------------
struct Kernel {
  const void* host = nullptr;   // a __global__ function of this library
  hipFunction_t mod = nullptr;  // or a function of a hipRTC module
  explicit operator bool() const { return host || mod; }
};
template <class... P>
Kernel kernel_of(void (*k)(P...)) {
  return Kernel{reinterpret_cast<const void*>(k), nullptr};
}

// args: the kernel's parameters, in its own types (their addresses are passed on, no copies)
template <class... Args>
hipError_t launch(const Kernel& k, dim3 g, dim3 b, hipStream_t s, const Args&... a) {
  void* args[] = {const_cast<void*>(static_cast<const void*>(&a))...};
  if (k.mod) return hipModuleLaunchKernel(k.mod, g.x, g.y, g.z, b.x, b.y, b.z, 0, s, args, nullptr);
  return hipLaunchKernel(k.host, g, b, args, 0, s);
}

struct Entry {
  int32_t model_id;
  int32_t S;
  int32_t P;  // the model's own parameter count
  // [method][traj][nt]; methods kAuto / kRosenbrock are null when S > kStiffMaxS, kBdf when
  // S > kStiffRegS
  Kernel integrate[kMethods][2][2];
  Kernel rk4_piped[3][2];  // [2, 4, 8 store waves][nt]; null when S > OE_PIPE_MAX_S
  Kernel dopri5_piped[2];  // [nt]: DOPRI5 trajectories through store waves; null when S > 6
  // 'auto' through the hand-over queue (S <= kHandMaxS): the DOPRI5 kernel, [beside][traj][nt]
  // (beside: its register budget leaves room for the BDF kernel on the same SIMDs), and the
  // BDF kernel, [beside][traj][nt] (after the DOPRI5 kernel: its difference table in registers)
  Kernel integrate_hq[2][2][2];
  Kernel bdf_hq[2][2][2];  // [beside][traj][nt]
  Kernel mh[kMethods];       // Metropolis–Hastings (mh.cuh), one lane per chain
  Kernel mh_init[kMethods];  // the a-priori pass (MHArgs::init)
  Kernel mh_tree[kMethods];  // speculative MH rounds (k_mh_tree); the resolve kernel is shared
  Kernel stiff_wave[2][2];   // [traj][nt]: S > kStiffRegS stiff redo, one wave per walker
  Kernel dopri5_split[2][2];  // [traj][nt]: DOPRI5 with split_lanes lanes per walker (split.cuh)
  Kernel mh_split;            // DOPRI5 Metropolis–Hastings, split_lanes lanes per walker (mh.cuh)
  Kernel mh_split_tree;       // its speculative rounds (k_mh_split_tree)
  int32_t split_lanes = 0;    // 0: the model has no split kernel
};

// lanes per walker of a model's split DOPRI5 kernel (split.cuh): the built-in chain only
template <class M>
struct SplitOf { static constexpr int K = 0; };
template <int N>
struct SplitOf<Chain<N>> { static constexpr int K = split_lanes_chain<N>(); };
#ifdef OE_SPLIT_TWOI  // measurement builds: two_i (Chain<4>'s RHS, operation for operation) over 2 or 4 lanes
static_assert(OE_SPLIT_TWOI == 2 || OE_SPLIT_TWOI == 4, "OE_SPLIT_TWOI: 2 or 4 lanes per walker (=2 or =4, not bare)");
template <>
struct SplitOf<TwoI> { static constexpr int K = OE_SPLIT_TWOI; };
#endif
// The split kernels are DOPRI5's only (mh_split / dopri5_split): no 'auto' / 'bdf' launch takes
// them, so the per-lane BDF pass and its deferred-observation scratch (DevProblem::obs_c,
// which oe_mh_run leaves null for split launches) never meet a split walker.

// [traj][nt] slots: the store policy only matters with a trajectory
inline void fill(Kernel (&slot)[2][2], Kernel chi_only, Kernel traj, Kernel traj_nt) {
  slot[0][0] = slot[0][1] = chi_only;
  slot[1][0] = traj;
  slot[1][1] = traj_nt;
}

template <class M, int METHOD>
void fill_method(Entry& e) {
  // 'auto' with S <= kHandMaxS integrates through the hand-over queue (integrate_hq / bdf_hq)
  if constexpr (!kHandQueue<M, METHOD>)
    fill(e.integrate[METHOD], kernel_of(k_integrate<M, METHOD, false, false>),
         kernel_of(k_integrate<M, METHOD, true, false>), kernel_of(k_integrate<M, METHOD, true, true>));
  // the stiff methods' MH chains with one lane per chain (S <= kStiffRegS) run as rounds of
  // k_mh_tree + k_mh_resolve, one iteration a round when not speculating (kMhRoundsOnly)
  if constexpr (!kMhRoundsOnly<M, METHOD>) e.mh[METHOD] = kernel_of(k_mh<M, METHOD, false>);
  e.mh_init[METHOD] = kernel_of(k_mh<M, METHOD, true>);
  e.mh_tree[METHOD] = kernel_of(k_mh_tree<M, METHOD>);
}

template <class M>
Entry make_entry(int32_t model_id) {
  Entry e{};
  e.model_id = model_id;
  e.S = M::S;
  e.P = M::P;
  fill_method<M, kRK4>(e);
  fill_method<M, kDOPRI5>(e);
  if constexpr (M::S <= kStiffMaxS) {
    fill_method<M, kAuto>(e);
    fill_method<M, kRosenbrock>(e);
  }
  if constexpr (M::S <= kStiffRegS) fill_method<M, kBdf>(e);
  if constexpr (M::S <= kHandMaxS) {
    fill(e.integrate_hq[1], kernel_of(k_integrate_hq<M, false, false, true>),
         kernel_of(k_integrate_hq<M, true, false, true>), kernel_of(k_integrate_hq<M, true, true, true>));
    fill(e.integrate_hq[0], kernel_of(k_integrate_hq<M, false, false, false>),
         kernel_of(k_integrate_hq<M, true, false, false>), kernel_of(k_integrate_hq<M, true, true, false>));
    fill(e.bdf_hq[1], kernel_of(k_bdf_hq<M, false, false, false>), kernel_of(k_bdf_hq<M, true, false, false>),
         kernel_of(k_bdf_hq<M, true, true, false>));
    fill(e.bdf_hq[0], kernel_of(k_bdf_hq<M, false, false, true>), kernel_of(k_bdf_hq<M, true, false, true>),
         kernel_of(k_bdf_hq<M, true, true, true>));
  }
  if constexpr (M::S <= 8 && dp_pipe_slots<M::S>() >= 2) {  // a slot ring of >= 2 steps fits (S <= 6)
    e.dopri5_piped[0] = kernel_of(k_integrate_dopri5_piped<M, false>);
    e.dopri5_piped[1] = kernel_of(k_integrate_dopri5_piped<M, true>);
  }
  if constexpr (M::S > kStiffRegS && M::S <= kStiffMaxS)
    fill(e.stiff_wave, kernel_of(k_stiff_wave<M, false, false>), kernel_of(k_stiff_wave<M, true, false>),
         kernel_of(k_stiff_wave<M, true, true>));
  if constexpr (SplitOf<M>::K > 0) {
    constexpr int K = SplitOf<M>::K;
    e.split_lanes = K;
    fill(e.dopri5_split, kernel_of(k_integrate_split<M::S, K, false, false>),
         kernel_of(k_integrate_split<M::S, K, true, false>), kernel_of(k_integrate_split<M::S, K, true, true>));
    e.mh_split = kernel_of(k_mh_split<M::S, K>);
    e.mh_split_tree = kernel_of(k_mh_split_tree<M::S, K>);
  }
  if constexpr (M::S <= OE_PIPE_MAX_S) {
    e.rk4_piped[0][0] = kernel_of(k_integrate_rk4_piped<M, false, 2>);
    e.rk4_piped[0][1] = kernel_of(k_integrate_rk4_piped<M, true, 2>);
    e.rk4_piped[1][0] = kernel_of(k_integrate_rk4_piped<M, false, 4>);
    e.rk4_piped[1][1] = kernel_of(k_integrate_rk4_piped<M, true, 4>);
    e.rk4_piped[2][0] = kernel_of(k_integrate_rk4_piped<M, false, 8>);
    e.rk4_piped[2][1] = kernel_of(k_integrate_rk4_piped<M, true, 8>);
  }
  return e;
}

}  // namespace oe

// one factory per instantiation unit
#define OE_DECLARE_ENTRY(NAME) oe::Entry oe_entry_##NAME()
