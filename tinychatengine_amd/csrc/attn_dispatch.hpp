// attn_dispatch.hpp -- what the launchers of attention_fast.hip and attention_prefill.hip share on the host: the form choice and the launch's status.
#pragma once
#include <type_traits>

#include "tce_common.hpp"

namespace tce {

// Runtime bools become the compile-time arguments of a generic callable: with_bools(f, x, y) calls f(std::bool_constant<x>{}, std::bool_constant<y>{}).  A kernel
// family's launch is then ONE statement inside f; the combinations of flags that are no form of the family are cut there with `if constexpr`, so that they are
// never instantiated.
template <class F>
void with_bools(F &&f) {
    f();
}
template <class F, class... Bools>
void with_bools(F &&f, bool b, Bools... rest) {
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// the tail of every launcher: TCE_OK, or TCE_ERR_HIP with the runtime's error in *hip_err
static int launch_status(hipError_t *hip_err) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return TCE_OK;
    if (hip_err) *hip_err = e;
    return TCE_ERR_HIP;
}

}  // namespace tce
