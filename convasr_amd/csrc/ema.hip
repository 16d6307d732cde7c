// Exponential moving average of the parameter arena (train.WeightEMA) and the in-place exchange of two device buffers.
//
// convasr_ema_update -- one streaming pass over n fp32 elements, in this operation order (tests/_ema_ref.py restates it):
//   k    = k_in[0]                                   updates APPLIED so far, a device float (saturates at 2^24)
//   skip = (loss_gate && !(|*loss_gate| < inf)) || (scaler_state && scaler_state[LS_OVERFLOW] != 0)
//   k_out[0] = skip ? k : min(k + 1, 2^24);  skip: nothing else is written -- not e, not the mirror
//   d    = min(decay, rn((1 + k) / (10 + k)))        fp32, correctly rounded sum, sum, quotient
//   omd  = rn(1 - d)
//   e'   = k == 0 ? w : fma(omd, rn(w - e), e)       two roundings per element: the difference, then the fused multiply-add
//   e16' = rn16(e')                                  round-to-nearest-even to bf16 / fp16, when a mirror is given
// The skip rule is the optimizers' own: sgd_step_kernel, adamw_step_kernel (misc.hip) and ng_step_kernel (next.hip) all return on
// `gated || ls.overflow`, gated from the same loss_gate expression, and loss_scale_advance (common.h) records ls.overflow of a step that
// was not gated in LS_OVERFLOW of the state it writes (a static scale, window 0, writes 0: it never skips) -- so the update that follows
// an optimizer step is handed that step's loss_gate and the scaler state the step WROTE, and skips exactly when the step did.  A gated
// step carries LS_OVERFLOW over from the step before; the gate alone already skips then.
// k_in != k_out: other workgroups read k while one thread writes the next value, so the two live in different buffers the caller swaps (or
// hands back with convasr_copy once a captured graph bakes the addresses), like convasr_adamw_step's step_in / step_out.
#include "common.h"

#define EMA_THREADS 256
#define EMA_SPAN (EMA_THREADS * 8)  // elements of one workgroup per grid pass: 8 per lane = two 16-byte loads per fp32 array, one 16-byte store of the mirror
#define EMA_MAX_BLOCKS 2048         // arenas beyond EMA_MAX_BLOCKS * EMA_SPAN elements loop

template <typename H> __global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const float* __restrict__ w, float* __restrict__ e, H* __restrict__ e16, int64_t n, float decay,
                                                                                      const float* __restrict__ k_in, float* __restrict__ k_out, const float* __restrict__ loss_gate,
                                                                                      const float* __restrict__ scaler_state) {
	const bool gated = loss_gate && !(fabsf(*loss_gate) < INFINITY);
	const bool skip = gated || (scaler_state && scaler_state[LS_OVERFLOW] != 0.f);
	const float k = *k_in;
	if (blockIdx.x == 0 && threadIdx.x == 0) *k_out = skip ? k : fminf(k + 1.f, 16777216.f);
	if (skip) return;
	const float d = fminf(decay, __fdiv_rn(__fadd_rn(1.f, k), __fadd_rn(10.f, k))), omd = __fsub_rn(1.f, d);
	const bool first = k == 0.f;
	for (int64_t i = ((int64_t)blockIdx.x * EMA_THREADS + threadIdx.x) * 8; i < n; i += (int64_t)gridDim.x * EMA_SPAN) {
		float r[8];
		load8<float>(w + i, r);
		if (!first) {  // (the first applied update copies: the average's old content is not read)
			float ev[8];
			load8<float>(e + i, ev);
#pragma unroll
			for (int j = 0; j < 8; ++j) r[j] = __fmaf_rn(omd, __fsub_rn(r[j], ev[j]), ev[j]);
		}
		store8<float>(e + i, r);
		if (e16) store8<H>(e16 + i, r);
	}
}

extern "C" int convasr_ema_update(const float* w, float* e, void* e16, int e16_dtype, int64_t n, float decay, const float* k_in, float* k_out, const float* loss_gate,
                                  const float* scaler_state, void* stream) {
	CONVASR_CHECK_ARG(w && e && w != e && k_in && k_out && k_in != k_out && n > 0 && n % 8 == 0, "ema_update: needs distinct w / e, distinct k_in / k_out and n > 0, a multiple of 8");
	CONVASR_CHECK_ARG(decay >= 0.f && decay <= 1.f, "ema_update: decay in [0, 1]");
	CONVASR_CHECK_ARG(!e16 || convasr_is_half(e16_dtype), "ema_update: the mirror's dtype must be CONVASR_BF16 or CONVASR_F16");
	CONVASR_CHECK_ARG((((uintptr_t)w | (uintptr_t)e | (uintptr_t)e16) & 15) == 0, "ema_update: w, e and the mirror must be 16-byte aligned");
	int64_t blocks = ceil_div64(n, EMA_SPAN);
	if (blocks > EMA_MAX_BLOCKS) blocks = EMA_MAX_BLOCKS;
	CONVASR_DISPATCH_HALF(e16_dtype, H, hipLaunchKernelGGL((ema_update_kernel<H>), dim3((unsigned)blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream, w, e, (H*)e16, n, decay, k_in, k_out, loss_gate, scaler_state));
	CONVASR_CHECK_LAUNCH("ema_update");
	return 0;
}

extern "C" int64_t convasr_ema_update_span(void) { return EMA_SPAN; }
extern "C" int64_t convasr_ema_update_max_blocks(void) { return EMA_MAX_BLOCKS; }

// a[0..nbytes) <-> b[0..nbytes): every lane owns its 16 bytes of both buffers, reads both, writes both -- no element is touched by two lanes.
#define SWAP_THREADS 256
#define SWAP_MAX_BLOCKS 2048
__global__ __launch_bounds__(SWAP_THREADS) void swap_kernel(uint4* __restrict__ a, uint4* __restrict__ b, int64_t n16) {
	for (int64_t i = (int64_t)blockIdx.x * SWAP_THREADS + threadIdx.x; i < n16; i += (int64_t)gridDim.x * SWAP_THREADS) {
		const uint4 va = a[i], vb = b[i];
		a[i] = vb;
		b[i] = va;
	}
}

extern "C" int convasr_swap(void* a, void* b, int64_t nbytes, void* stream) {
	CONVASR_CHECK_ARG(a && b && nbytes > 0 && nbytes % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0, "swap: needs two 16-byte aligned buffers of a multiple of 16 bytes");
	const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
	CONVASR_CHECK_ARG(pa + (uintptr_t)nbytes <= pb || pb + (uintptr_t)nbytes <= pa, "swap: the buffers overlap");
	const int64_t n16 = nbytes / 16;
	int64_t blocks = ceil_div64(n16, SWAP_THREADS);
	if (blocks > SWAP_MAX_BLOCKS) blocks = SWAP_MAX_BLOCKS;
	hipLaunchKernelGGL(swap_kernel, dim3((unsigned)blocks), dim3(SWAP_THREADS), 0, (hipStream_t)stream, (uint4*)a, (uint4*)b, n16);
	CONVASR_CHECK_LAUNCH("swap");
	return 0;
}

extern "C" int64_t convasr_swap_span_bytes(void) { return SWAP_THREADS * 16; }
