// split_bf16.h — an f32 number as the sum of two bf16 numbers and a remainder of at most 2^-16 of it: the operands of the
// split-bf16 score tile (k_exact_scores_bf16x3, exact_split_kernels.h; the bound that rests on it: exact_certificate.h).
//
// Pure functions of plain numbers — no HIP types — compiled for the device and, by tests/exact_split_probe.cpp, for the host.
//
//   hi = bf16(x)                 round to nearest, ties to even:  |x - hi| <= 2^-8 |x|   (bf16 carries 8 significant bits)
//   lo = bf16(x - float(hi))     the subtraction is exact in f32 (x and hi agree in sign and exponent up to one binade, the
//                                difference has at most 16 significant bits):  |x - hi - lo| <= 2^-8 |x - hi| <= 2^-16 |x|
// For finite normal inputs these are the bits v_cvt_pk_bf16_f32 (gfx950) gives, which the kernels use.  +-inf stays +-inf in hi
// (lo is then NaN), a NaN stays a NaN, and an f32 above the largest bf16 rounds to inf: none of these can be certified
// (exact_cert_error_split's guards on the norms).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSS_SPLIT_HD __host__ __device__
#else
#define VSS_SPLIT_HD
#endif

namespace vss {

VSS_SPLIT_HD inline uint32_t split_bf16_bits(float x) {
	uint32_t b;
	memcpy(&b, &x, 4);
	return b;
}
VSS_SPLIT_HD inline float split_bf16_float(uint32_t b) {
	float x;
	memcpy(&x, &b, 4);
	return x;
}

// the bf16 nearest to x (ties to even), as its 16-bit pattern
VSS_SPLIT_HD inline uint16_t bf16_round(float x) {
	const uint32_t b = split_bf16_bits(x);
	if ((b & 0x7F800000u) == 0x7F800000u) // inf stays inf; a NaN keeps a set mantissa bit
		return (uint16_t)((b >> 16) | ((b & 0x007FFFFFu) ? 0x0040u : 0u));
	return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}
// the f32 value of a bf16 pattern
VSS_SPLIT_HD inline float bf16_value(uint16_t h) {
	return split_bf16_float((uint32_t)h << 16);
}

struct SplitBf16 {
	uint16_t hi, lo;
};
VSS_SPLIT_HD inline SplitBf16 split_bf16(float x) {
	SplitBf16 s;
	s.hi = bf16_round(x);
	s.lo = bf16_round(x - bf16_value(s.hi));
	return s;
}

} // namespace vss
