// dqnhip_test_gemm_form (gemm_forms.hip: the same validation, buffers and product launcher) in a library of its own whose launches
// can go out on a LaunchOn with no_preload set — what DQNHIP_TUNE_NO_KERNARG_PRELOAD does in the learner: the launchers then mark the
// GemmPreload block "not valid" and the chain kernels take their GemmArgs path.  dqnhip_test_set_no_preload(1 / 0) switches it.
// tests/test_gpu_kernarg_preload.py builds this file WITH the preload option (libdqnhip_test.so and its Makefile are as they were:
// there the option is off and the leading words arrive by scalar loads), so here, bit clear or set, they really arrive in SGPRs.
#include "gemm_direct.hip.h"

namespace dqnhip {
static bool g_no_preload = false;
inline LaunchOn test_launch_on(hipStream_t s) { LaunchOn on(s); on.no_preload = g_no_preload; return on; }
}  // namespace dqnhip
extern "C" void dqnhip_test_set_no_preload(int off) { dqnhip::g_no_preload = off != 0; }

// (after the product header, so that only the CALL in gemm_forms.hip is rewritten)
#define gemm_form_launch(form, b, s) gemm_form_launch(form, b, ::dqnhip::test_launch_on(s))
#include "gemm_forms.hip"
#undef gemm_form_launch
