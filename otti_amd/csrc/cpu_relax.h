// The one instruction every spinning host loop of the library issues between two polls.  Host only, no HIP include: the plain-compiler
// builds of the host sources (tests/san, tools/roundbench) take it as it is.
#pragma once
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace otti {
inline void cpu_relax() {
#if defined(__x86_64__)
    _mm_pause();
#endif
}
}  // namespace otti
