// rtc.h — user right-hand sides compiled at run time (see rtc.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace oe {

struct Entry;  // dispatch.h

// The modules of one user RHS, built in two parts on demand: the explicit methods (RK4,
// DOPRI5) when the model is compiled, the stiff ones (auto, Rosenbrock, BDF: the body
// instantiated with dual numbers, plus the one-wave-per-walker kernel for S > 8) the first
// time a problem asks for them.  Their kernels go into the model's own Entry.
struct RtcModule {
  hipModule_t mod = nullptr;        // RK4 + DOPRI5
  hipModule_t stiff_mod = nullptr;  // auto + Rosenbrock + BDF (+ k_stiff_wave)
  int stiff = 0;                    // 0: not built yet, 1: built, -1: unavailable (stiff_err)
  std::string stiff_err;
};

enum RtcPart { kRtcExplicit = 0, kRtcStiff = 1 };

// Compile (and, if out != null, load into *out, filling the part's slots of *entry) one part
// of the kernels of a user RHS body; 0 on success, else -1 with the compiler log in err.  The stiff part needs
// S <= kStiffMaxS and a body that compiles for dual numbers (templated on R, no `double`
// temporaries).
int rtc_build(const std::string& body, int S, int P, const char* arch, RtcPart part, RtcModule* out,
              Entry* entry, std::string& err);

}  // namespace oe
