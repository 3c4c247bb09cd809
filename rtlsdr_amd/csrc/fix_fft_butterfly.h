// fix_fft_butterfly.h — fix_fft's arithmetic (reference src/rtl_power.c:263-327) on packed int16 pairs: FIX_MPY and one
// radix-2 butterfly.  Shared by rtl_power's transforms (power_kernels.h) and the channel bank (channel_bank_kernel.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlpower {

// FIX_MPY, src/rtl_power.c:263-269
__device__ __forceinline__ int fix_mpy(int a, int b)
{
	int c = (a * b) >> 14;
	return (int)(int16_t)((c >> 1) + (c & 1));
}

typedef short pk16_t __attribute__((ext_vector_type(2)));

// One butterfly of fix_fft (src/rtl_power.c:309-321) on packed (re, im) int16 pairs.
//   FIX_MPY(a, b) = ((a*b >> 14) >> 1) + ((a*b >> 14) & 1) = (a*b + 2^14) >> 15 = (a*2b + 2^15) >> 16  (exact)
//   tr = FIX_MPY(wr, b.re) - FIX_MPY(wi, b.im), ti = FIX_MPY(wr, b.im) + FIX_MPY(wi, b.re)
//   q  = a >> 1 (per component);  b' = q - t,  a' = q + t
// Every int16 store of the reference wraps mod 2^16; so do the packed 16-bit adds here.
// The twiddle table holds (2 wr, 2 wi) (both fit int16: wr, wi are the halved sines, -16384 .. 16383), so
// every FIX_MPY is the HIGH HALF of one v_mad_i32_i16 - op_sel takes the 16-bit halves straight out of the
// packed twiddle and the packed point, the rounding constant is the addend - and two v_perm gather the
// four high halves into the packed pairs (m1, m3) and (m2, m4) without a single shift; the one subtraction
// among tr, ti is a packed multiply-add by (-1, +1).  10 instructions per butterfly: 4 v_mad_i32_i16,
// 2 v_perm, v_pk_mad_i16, v_pk_ashr, v_pk_sub, v_pk_add (rounds 1-2: 18, round 3 before this: 14).
__device__ __forceinline__ int mad_i16(uint32_t x, uint32_t y, int c, int xhi, int yhi)
{
	int r;
	if (!xhi && !yhi) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,0,0,0]" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	else if (xhi && yhi) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,1,0,0]" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	else if (yhi) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,1,0,0]" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	else asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(r) : "v"(x), "v"(y), "s"(c));
	return r;
}
// KIND: 0 = any twiddle; 1 = the twiddle is real (wi == 0: FIX_MPY(0, x) == 0, two products drop out);
// 2 = it is imaginary (wr == 0).  The first three stages know which at compile time: positions 0 and N/4.
template <int KIND = 0>
__device__ __forceinline__ void butterfly(uint32_t &a, uint32_t &b, uint32_t w2)
{
	const pk16_t pm = {(short)-1, (short)1};  // t = (m1 - m2, m3 + m4) = (m2, m4) * (-1, +1) + (m1, m3): one v_pk_mad_i16
	pk16_t tv;
	if (KIND == 1) {
		const uint32_t p1 = (uint32_t)mad_i16(w2, b, 32768, 0, 0);  // high half: FIX_MPY(wr, b.re)
		const uint32_t p3 = (uint32_t)mad_i16(w2, b, 32768, 0, 1);  //            FIX_MPY(wr, b.im)
		tv = __builtin_bit_cast(pk16_t, __builtin_amdgcn_perm(p3, p1, 0x07060302u));
	} else {
		const uint32_t p2 = (uint32_t)mad_i16(w2, b, 32768, 1, 1);  // FIX_MPY(wi, b.im)
		const uint32_t p4 = (uint32_t)mad_i16(w2, b, 32768, 1, 0);  // FIX_MPY(wi, b.re)
		const pk16_t m24 = __builtin_bit_cast(pk16_t, __builtin_amdgcn_perm(p4, p2, 0x07060302u));
		if (KIND == 0) {
			const uint32_t p1 = (uint32_t)mad_i16(w2, b, 32768, 0, 0);  // FIX_MPY(wr, b.re)
			const uint32_t p3 = (uint32_t)mad_i16(w2, b, 32768, 0, 1);  // FIX_MPY(wr, b.im)
			const pk16_t m13 = __builtin_bit_cast(pk16_t, __builtin_amdgcn_perm(p3, p1, 0x07060302u));
			tv = m24 * pm + m13;
		} else {
			tv = m24 * pm;
		}
	}
	const pk16_t q = __builtin_bit_cast(pk16_t, a) >> 1;
	b = __builtin_bit_cast(uint32_t, (pk16_t)(q - tv));
	a = __builtin_bit_cast(uint32_t, (pk16_t)(q + tv));
}

}  // namespace rtlpower
