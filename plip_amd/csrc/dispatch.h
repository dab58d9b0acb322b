// dispatch.h -- host only: a launcher's dtype code (kernels.h: 0 = fp32, 1 = bf16, 2 = f16) turned into the operand type, in one
// place: with_half(dtype, [&](auto tag) { using H = decltype(tag); hipLaunchKernelGGL(k<H>, ...); }).  Neither function checks the
// code -- every launcher validates its arguments first, with its own return codes -- so the last arm takes whatever is left: f16
// for with_half, fp32 for with_dtype.  What the callback returns is returned.
// with_pad(pad, [&](auto tag) { constexpr int DP = decltype(tag)::value; ... }) does the same for the head size the attention
// kernels are instantiated at (kernels.h attention_head_pad: 64, or the padded sizes 96 and 128 that carry heads of 72 .. 128).
#pragma once
#include "common.h"

namespace plipmi {

template <typename F>
inline decltype(auto) with_half(int dtype, F&& f) {
  return dtype == 1 ? f(bf16_t{}) : f(f16_t{});
}
template <typename F>
inline decltype(auto) with_dtype(int dtype, F&& f) {
  return dtype == 1 ? f(bf16_t{}) : dtype == 2 ? f(f16_t{}) : f(float{});
}
template <int N> struct pad_tag { static constexpr int value = N; };
template <typename F>
inline decltype(auto) with_pad(int pad, F&& f) {
  return pad == 64 ? f(pad_tag<64>{}) : pad == 96 ? f(pad_tag<96>{}) : f(pad_tag<128>{});
}

}  // namespace plipmi
