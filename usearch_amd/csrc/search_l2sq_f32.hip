// usearch_amd/csrc/search_l2sq_f32.hip — kernel instantiations for metric l2sq over f32 storage (launch_impl.hpp).
#include "launch_impl.hpp"
namespace usearch_amd {
USEARCH_AMD_DEFINE_LAUNCHERS(l2sq_f32, metric_l2sq_k, scalar_f32_k)
USEARCH_AMD_DEFINE_SCREENED_LAUNCHER(l2sq_f32, metric_l2sq_k, scalar_f32_k)
}
