// Primitives over the 64 lanes of a wave, and the length clamp every per-utterance kernel starts with (included by common.h).
#pragma once

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
	return v;
}
// the same butterfly for 64-bit (value, index) keys
__device__ __forceinline__ long long wave_max(long long k) {
	for (int off = 32; off >= 1; off >>= 1) {
		const long long o = __shfl_xor(k, off);
		k = o > k ? o : k;
	}
	return k;
}

// DPP move with bound_ctrl off: a lane whose source lies outside its row, or whose row is masked off, gets `old`
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int wave_dpp(int old, int src) {
	return __builtin_amdgcn_update_dpp(old, src, CTRL, ROWS, 0xf, false);
}

// Inclusive prefix minimum / maximum / sum (modulo 2^32) over the 64 lanes: row_shr 1, 2, 4, 8 inside each row of 16, then the two row
// broadcasts; no LDS round trip.  `fill` is the operation's identity over the values the caller scans (a literal at every call site).
__device__ __forceinline__ int wave_prefix_min(int x, int fill) {
	x = min(x, wave_dpp<0x111>(fill, x));
	x = min(x, wave_dpp<0x112>(fill, x));
	x = min(x, wave_dpp<0x114>(fill, x));
	x = min(x, wave_dpp<0x118>(fill, x));
	x = min(x, wave_dpp<0x142, 0xa>(fill, x));  // row_bcast:15 into rows 1 and 3
	x = min(x, wave_dpp<0x143, 0xc>(fill, x));  // row_bcast:31 into rows 2 and 3
	return x;
}
__device__ __forceinline__ int wave_prefix_max(int x, int fill) {
	x = max(x, wave_dpp<0x111>(fill, x));
	x = max(x, wave_dpp<0x112>(fill, x));
	x = max(x, wave_dpp<0x114>(fill, x));
	x = max(x, wave_dpp<0x118>(fill, x));
	x = max(x, wave_dpp<0x142, 0xa>(fill, x));
	x = max(x, wave_dpp<0x143, 0xc>(fill, x));
	return x;
}
__device__ __forceinline__ int wave_prefix_sum(int x, int fill) {
	x += wave_dpp<0x111>(fill, x);
	x += wave_dpp<0x112>(fill, x);
	x += wave_dpp<0x114>(fill, x);
	x += wave_dpp<0x118>(fill, x);
	x += wave_dpp<0x142, 0xa>(fill, x);
	x += wave_dpp<0x143, 0xc>(fill, x);
	return x;
}

// lane i <- lane i - 1 (lane 0 <- fill) / lane i <- lane i + 1 (lane 63 <- fill): one DPP move (wave_shr:1 is wave_dpp<0x138>), no LDS
// round trip
__device__ __forceinline__ float wave_shr1(float v, float fill) {
	return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v, float fill) {
	return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

__device__ __forceinline__ int lane_rank(uint64_t mask) {  // set bits of mask below this lane
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ int clamp_len(int64_t n, int hi) { return n < 0 ? 0 : n > hi ? hi : (int)n; }
