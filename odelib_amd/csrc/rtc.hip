// rtc.hip — run-time compilation of user right-hand sides (hipRTC).
//
// The reference integrates any user Python callable ODE(y, t, ps) (Framework.py:177-180,
// :656).  Built-in models are compiled ahead of time (models.cuh); any other RHS is
// given as the body of
//     template <class R> __device__ void rhs(const R* y, R t, const R* ps, R* dy)
// (C source, or transpiled from the Python callable by odelib_amd/transpile.py) and the
// SAME kernel templates (ode_kernels.cuh, embedded at build time) are instantiated for
// it with hiprtc for the device's gfx950 target, loaded as a module and launched with
// hipModuleLaunchKernel.  The explicit methods are compiled with the model; the stiff
// ones (dual-number Jacobian, the larger kernels) only when a problem first asks for them.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "dispatch.h"
#include "rtc.h"
#include "rtc_source.inc"

namespace oe {

static const char* kBool[2] = {"false", "true"};

// k_mh's iteration loop for method m (mh.cuh kMhRoundsOnly: the stiff methods of
// register-path models run their chains as k_mh_tree rounds only)
static bool has_mh_loop(int S, int m) { return !((m == kAuto || m == kBdf) && S <= kStiffRegS); }

// The kernels of a part — RK4 + DOPRI5; auto + Rosenbrock (+ BDF up to kStiffRegS states, +
// k_stiff_wave above) — each visited as f(name expression, type of its second parameter, its
// slot in e).  The one list behind the generated instantiations, the name expressions and
// the module lookups.
template <class F>
static bool for_each_kernel(int S, RtcPart part, Entry& e, F&& f) {
  const bool stiff = part == kRtcStiff;
  const int m0 = stiff ? kAuto : kRK4, m1 = stiff ? (S <= kStiffRegS ? kBdf : kRosenbrock) : kDOPRI5;
  for (int m = m0; m <= m1; ++m) {
    const std::string mm = "<UserModel, " + std::to_string(m);
    for (int tr = 0; tr < 2; ++tr)
      for (int nt = 0; nt < 2; ++nt)
        if (!f("oe::k_integrate" + mm + ", " + kBool[tr] + ", " + kBool[nt] + ">", "IntegrateArgs", e.integrate[m][tr][nt]))
          return false;
    if (has_mh_loop(S, m) && !f("oe::k_mh" + mm + ">", "MHArgs", e.mh[m])) return false;
    if (!f("oe::k_mh" + mm + ", true>", "MHArgs", e.mh_init[m])) return false;
    if (!f("oe::k_mh_tree" + mm + ">", "MHTreeArgs", e.mh_tree[m])) return false;
  }
  if (stiff && S > kStiffRegS)
    for (int tr = 0; tr < 2; ++tr)
      for (int nt = 0; nt < 2; ++nt)
        if (!f(std::string("oe::k_stiff_wave<UserModel, ") + kBool[tr] + ", " + kBool[nt] + ">", "StiffWaveArgs",
               e.stiff_wave[tr][nt]))
          return false;
  return true;
}

std::string rtc_source(const std::string& body, int S, int P, RtcPart part) {
  std::string src;
  src += "typedef unsigned long long uint64_t; typedef long long int64_t;\n";
  src += "typedef unsigned int uint32_t; typedef int int32_t;\n";
  src += kRtcKernelSource;
  char hdr[256];
  snprintf(hdr, sizeof(hdr), "\nstruct UserModel {\n  static constexpr int S = %d, P = %d;\n", S, P);
  src += hdr;
  src += "  template <class R>\n  __device__ static inline void rhs(const R* y, R t, const R* ps, R* dy) {\n";
  src += "    (void)t;\n";
  src += body;
  src += "\n  }\n};\n";
  Entry none{};
  for_each_kernel(S, part, none, [&](const std::string& name, const char* args, Kernel&) {
    src += "template __global__ void " + name + "(const oe::DevProblem, const oe::" + args + ");\n";
    return true;
  });
  return src;
}

// lowered: name expression -> the kernel's symbol in the code object
static int compile_program(const std::string& src, const char* arch, const std::vector<std::string>& names,
                           std::map<std::string, std::string>& lowered, std::vector<char>& code, std::string& log) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "odelib_user_rhs.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
    log = "hiprtcCreateProgram failed";
    return -1;
  }
  for (auto& n : names) hiprtcAddNameExpression(prog, n.c_str());
  std::string archopt = std::string("--offload-arch=") + arch;
  const char* opts[] = {archopt.c_str(), "-O3", "-ffp-contract=off", "-std=c++17"};
  const hiprtcResult r = hiprtcCompileProgram(prog, 4, opts);
  size_t ls = 0;
  hiprtcGetProgramLogSize(prog, &ls);
  log.assign(ls, '\0');
  if (ls) hiprtcGetProgramLog(prog, &log[0]);
  if (r != HIPRTC_SUCCESS) {
    hiprtcDestroyProgram(&prog);
    return -1;
  }
  for (auto& n : names) {
    const char* lw = nullptr;
    if (hiprtcGetLoweredName(prog, n.c_str(), &lw) != HIPRTC_SUCCESS || !lw) {
      log += "\nno lowered name for " + n;
      hiprtcDestroyProgram(&prog);
      return -1;
    }
    lowered[n] = lw;
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  code.resize(cs);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  return 0;
}

int rtc_build(const std::string& body, int S, int P, const char* arch, RtcPart part, RtcModule* out,
              Entry* entry, std::string& err) {
  if (part == kRtcStiff && S > kStiffMaxS) {
    err = "the stiff methods (auto, rosenbrock) need n_states <= " + std::to_string(kStiffMaxS);
    return -1;
  }
  Entry none{};
  std::vector<std::string> names;
  for_each_kernel(S, part, none, [&](const std::string& name, const char*, Kernel&) {
    names.push_back(name);
    return true;
  });
  std::map<std::string, std::string> lowered;
  std::vector<char> code;
  std::string log;
  if (compile_program(rtc_source(body, S, P, part), arch, names, lowered, code, log)) {
    err = part == kRtcStiff
              ? "the stiff methods (auto, rosenbrock) need a right-hand side that compiles for dual numbers "
                "(templated on its scalar type R); hipRTC said:\n" + log
              : "hipRTC compilation of the user RHS failed:\n" + log;
    return -1;
  }
  if (!out) return 0;  // compile check only
  hipModule_t mod;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess) {
    err = "hipModuleLoadData failed for the user RHS";
    return -1;
  }
  (part == kRtcStiff ? out->stiff_mod : out->mod) = mod;
  if (!for_each_kernel(S, part, *entry, [&](const std::string& name, const char*, Kernel& slot) {
        return hipModuleGetFunction(&slot.mod, mod, lowered.at(name).c_str()) == hipSuccess;
      })) {
    err = "hipModuleGetFunction failed for the user RHS";
    return -1;
  }
  if (part == kRtcStiff) out->stiff = 1;
  return 0;
}

}  // namespace oe
