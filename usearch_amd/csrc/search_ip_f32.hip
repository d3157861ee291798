// usearch_amd/csrc/search_ip_f32.hip — kernel instantiations for metric ip over f32 storage (launch_impl.hpp).
#include "launch_impl.hpp"
namespace usearch_amd {
USEARCH_AMD_DEFINE_LAUNCHERS(ip_f32, metric_ip_k, scalar_f32_k)
USEARCH_AMD_DEFINE_SCREENED_LAUNCHER(ip_f32, metric_ip_k, scalar_f32_k)
}
