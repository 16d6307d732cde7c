// Training-time augmentation of a collated batch on the GPU: speed perturbation, gain and noise mixing on the waveforms (convasr_augment_params,
// convasr_augment_waveform, convasr_augment_mix) and SpecAugment on the log-mel features (convasr_spec_augment).  The rules live in
// include/convasr_hip.h; this is the project's own augmentation, unpinned against any outside library.
//
// Every random decision is word 0 of one Philox4x32-10 block: counter = (key low word, key high word, epoch, purpose << 16 | index), Philox key =
// (seed low word, seed high word).  Words become numbers by integer arithmetic only, so the host restatement (tests/_augment_ref.py) reproduces
// every decision exactly.  No kernel here calls a transcendental function: gains, SNR factors and the filter come from tables that the host
// computed in float64 and rounded once.
//
// Waveform pass.  A workgroup of AUG_THREADS threads owns the tiles part, part + nparts, ... of one utterance (nparts = min(tiles, AUG_PARTS)),
// AUG_TILE consecutive outputs each.  An utterance whose speed is not 1 loads its speed's table -- taps x (AUG_PHASES + 1) coefficients --
// into LDS once and, per tile, the input span the tile reads; every lane then walks the taps in ascending input index, one linear
// interpolation between the two neighbouring phases and one fma per tap.  The sums of squares of signal and noise window are kept per lane in
// float64, reduced once per workgroup in a fixed tree and left as one pair per workgroup; the mix pass adds the pairs in index order.  No atomics.
#include "common.h"

#define AUG_THREADS 256
#define AUG_TILE 1024                // outputs per tile: four per lane, each a coalesced row of 256
#define AUG_PBITS 7
#define AUG_PHASES (1 << AUG_PBITS)  // phases per input sample; the table holds AUG_PHASES + 1 columns (the last is phase 1.0 = the next tap's phase 0)
#define AUG_PW (AUG_PHASES + 1)
#define AUG_PARTS 32                 // workgroups (and partial sums) per utterance at most
#define AUG_MAX_SPEEDS 32
#define AUG_MAX_STEPS 4096           // gain and SNR table sizes
#define AUG_ONE (1ull << 32)         // speed 1.0 in 32.32 fixed point
#define AUG_LDS_MAX (160 * 1024)
#define AUG_RED_DOUBLES 8            // >= AUG_THREADS / 64
#define AUG_PARAMS 8                 // int64 per utterance: the fields below
enum { AP_SPEED = 0, AP_STEP = 1, AP_GAIN = 2, AP_NOISE = 3, AP_OFFSET = 4, AP_SNR = 5, AP_LEN = 6, AP_OUT_LEN = 7 };
// purposes (the high half of counter word 3)
enum { AS_SPEED_FIRE = 0, AS_SPEED = 1, AS_GAIN_FIRE = 2, AS_GAIN = 3, AS_NOISE_FIRE = 4, AS_NOISE_ROW = 5, AS_NOISE_OFFSET = 6, AS_SNR = 7, AS_FREQ_WIDTH = 8, AS_FREQ_START = 9, AS_TIME_WIDTH = 10, AS_TIME_START = 11 };

#define SPEC_THREADS 1024            // = elements one workgroup of convasr_spec_augment takes per step
#define SPEC_MAX_MASKS 16            // of each kind
#define SPEC_MAX_SPLIT 8             // workgroups per utterance at most

// Philox4x32-10 (Salmon et al. 2011, Random123): ten rounds of two 32 x 32 -> 64 multiplies, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ void aug_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
#pragma unroll
	for (int i = 0; i < 10; ++i) {
		const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
		const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
		const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
		c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
	r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// the random word of (seed, epoch, key, purpose, index)
__device__ __forceinline__ unsigned aug_draw(uint64_t seed, unsigned epoch, uint64_t key, unsigned purpose, unsigned index) {
	unsigned r[4];
	aug_philox((unsigned)key, (unsigned)(key >> 32), epoch, (purpose << 16) | (index & 0xffffu), (unsigned)seed, (unsigned)(seed >> 32), r);
	return r[0];
}
// a uniform integer in [0, n], n < 2^40
__device__ __forceinline__ int64_t aug_uint(unsigned r, int64_t n) { return (int64_t)(((uint64_t)(r >> 8) * (uint64_t)(n + 1)) >> 24); }
// fires with probability thr / 2^24
__device__ __forceinline__ bool aug_fires(unsigned r, unsigned thr) { return (r >> 8) < thr; }

__global__ __launch_bounds__(256) void philox_kernel(const int64_t* __restrict__ counters, int64_t n, unsigned k0, unsigned k1, int64_t* __restrict__ out) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	unsigned r[4];
	aug_philox((unsigned)counters[4 * i], (unsigned)counters[4 * i + 1], (unsigned)counters[4 * i + 2], (unsigned)counters[4 * i + 3], k0, k1, r);
#pragma unroll
	for (int j = 0; j < 4; ++j) out[4 * i + j] = (int64_t)r[j];
}

struct AugSteps { uint64_t v[AUG_MAX_SPEEDS]; };

__global__ __launch_bounds__(256) void augment_params_kernel(const float* __restrict__ xlen, const int64_t* __restrict__ keys, const int64_t* __restrict__ min_out_len, int B, int64_t T,
                                                             uint64_t seed, unsigned epoch, AugSteps steps, int n_speeds, unsigned speed_thr, int gain_steps, unsigned gain_thr,
                                                             int64_t noise_rows, int64_t noise_len, int snr_steps, unsigned noise_thr, int64_t* __restrict__ params, float* __restrict__ xlen_out) {
	const int b = blockIdx.x * 256 + threadIdx.x;
	if (b >= B) return;
	const uint64_t key = (uint64_t)keys[b];
	int64_t len = (int64_t)ceilf(xlen[b] * (float)T);  // ops.output_lengths' rule
	len = len < 0 ? 0 : (len > T ? T : len);
	int64_t speed = aug_uint(aug_draw(seed, epoch, key, AS_SPEED, 0), n_speeds - 1);
	uint64_t step = steps.v[speed];
	int64_t out_len = (int64_t)(((uint64_t)len << 32) / step);
	if (!aug_fires(aug_draw(seed, epoch, key, AS_SPEED_FIRE, 0), speed_thr) || out_len > T || (min_out_len != nullptr && out_len < min_out_len[b])) {
		speed = -1; step = AUG_ONE; out_len = len;
	}
	int64_t gain = -1, row = -1, offset = 0, snr = 0;
	if (gain_steps > 0 && aug_fires(aug_draw(seed, epoch, key, AS_GAIN_FIRE, 0), gain_thr)) gain = aug_uint(aug_draw(seed, epoch, key, AS_GAIN, 0), gain_steps - 1);
	if (noise_rows > 0 && aug_fires(aug_draw(seed, epoch, key, AS_NOISE_FIRE, 0), noise_thr)) {
		row = aug_uint(aug_draw(seed, epoch, key, AS_NOISE_ROW, 0), noise_rows - 1);
		offset = aug_uint(aug_draw(seed, epoch, key, AS_NOISE_OFFSET, 0), noise_len - 1);
		snr = aug_uint(aug_draw(seed, epoch, key, AS_SNR, 0), snr_steps - 1);
	}
	int64_t* p = params + (int64_t)b * AUG_PARAMS;
	p[AP_SPEED] = speed; p[AP_STEP] = (int64_t)step; p[AP_GAIN] = gain; p[AP_NOISE] = row; p[AP_OFFSET] = offset; p[AP_SNR] = snr; p[AP_LEN] = len; p[AP_OUT_LEN] = out_len;
	xlen_out[b] = __fdiv_rn((float)out_len, (float)T);
}

template <bool I16> __device__ __forceinline__ float aug_sample(const void* __restrict__ row, int64_t len, int64_t k) {
	if (k < 0 || k >= len) return 0.f;
	if (I16) return __fdiv_rn((float)((const int16_t*)row)[k], 32767.f);
	return ((const float*)row)[k];
}

// the sum of v over the workgroup's lanes in a fixed tree (xor butterfly inside a wave, the waves in ascending order); valid in lane 0 of wave 0
__device__ __forceinline__ double aug_block_sum(double v, double* red, int nwaves) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	double s = red[0];
	for (int w = 1; w < nwaves; ++w) s += red[w];
	return s;
}

// the row of this utterance's parameters, every field forced into the range the kernels index with (a caller may hand in its own tensor)
struct AugRow { int64_t speed, gain, noise, offset, snr, len, out_len; uint64_t step; };
__device__ __forceinline__ AugRow aug_row(const int64_t* __restrict__ params, int b, int64_t T, int n_speeds, int gain_steps, int64_t noise_rows, int64_t noise_len, int snr_steps) {
	const int64_t* p = params + (int64_t)b * AUG_PARAMS;
	AugRow r;
	r.speed = p[AP_SPEED]; r.step = (uint64_t)p[AP_STEP]; r.gain = p[AP_GAIN]; r.noise = p[AP_NOISE]; r.offset = p[AP_OFFSET]; r.snr = p[AP_SNR]; r.len = p[AP_LEN]; r.out_len = p[AP_OUT_LEN];
	r.len = r.len < 0 ? 0 : (r.len > T ? T : r.len);
	r.out_len = r.out_len < 0 ? 0 : (r.out_len > T ? T : r.out_len);
	if (n_speeds >= 0) {  // (the mix pass passes -1: it reads no speed)
		if (r.speed < 0 || r.speed >= n_speeds || r.step < (AUG_ONE >> 1) || r.step > (AUG_ONE << 1)) { r.speed = -1; r.step = AUG_ONE; }
		if (r.step == AUG_ONE && r.out_len > r.len) r.out_len = r.len;
	}
	if (r.gain >= gain_steps) r.gain = -1;
	if (r.noise >= noise_rows || r.offset < 0 || r.offset >= noise_len || r.snr < 0 || r.snr >= snr_steps) r.noise = -1;
	return r;
}

template <bool I16>
__global__ __launch_bounds__(AUG_THREADS) void augment_waveform_kernel(const void* __restrict__ x, const int64_t* __restrict__ params, const float* __restrict__ table, int n_speeds, int taps,
                                                                       const float* __restrict__ gain_table, int gain_steps, const float* __restrict__ noise, int64_t noise_rows, int64_t noise_len,
                                                                       float* __restrict__ out, double* __restrict__ partials, int64_t T, int64_t ntiles) {
	// [the reduction's scratch][taps * AUG_PW coefficients of this utterance's speed][the input span of a tile] -- all of it dynamic: with a static
	// array beside it the kernel could not be granted the device's whole 160 KiB
	extern __shared__ double aug_lds_base[];
	double* red = aug_lds_base;
	float* aug_lds = (float*)(aug_lds_base + AUG_RED_DOUBLES);
	const int tid = threadIdx.x, b = blockIdx.y, part = blockIdx.x, nparts = gridDim.x, H = taps / 2 - 1;
	const AugRow r = aug_row(params, b, T, taps > 0 ? n_speeds : 0, gain_steps, noise_rows, noise_len, AUG_MAX_STEPS);
	const bool resamp = r.step != AUG_ONE;
	const void* xrow = I16 ? (const void*)((const int16_t*)x + (int64_t)b * T) : (const void*)((const float*)x + (int64_t)b * T);
	float* orow = out + (int64_t)b * T;
	float* xs = aug_lds + taps * AUG_PW;
	if (resamp) {
		const float* tg = table + r.speed * (int64_t)taps * AUG_PW;
		for (int i = tid; i < taps * AUG_PW; i += AUG_THREADS) aug_lds[i] = tg[i];  // (the barrier after the span's fill covers it)
	}
	const float g = r.gain >= 0 ? gain_table[r.gain] : 1.f;
	const float* nz = (noise != nullptr && r.noise >= 0) ? noise + r.noise * noise_len : nullptr;
	const int64_t dm = AUG_THREADS % (nz ? noise_len : 1);
	double ex = 0.0, en = 0.0;
	for (int64_t tile = part; tile < ntiles; tile += nparts) {
		const int64_t n0 = tile * AUG_TILE;
		if (n0 >= r.out_len) {  // (uniform over the workgroup)
			for (int i = 0; i < AUG_TILE / AUG_THREADS; ++i) { const int64_t n = n0 + tid + i * AUG_THREADS; if (n < T) orow[n] = 0.f; }
			continue;
		}
		const int64_t n_last = min(n0 + AUG_TILE, r.out_len) - 1;
		int64_t kb = 0;
		if (resamp) {
			kb = (int64_t)(((uint64_t)n0 * r.step) >> 32) - H;                                    // first input index any output of the tile reads
			const int span = (int)((int64_t)(((uint64_t)n_last * r.step) >> 32) + H + 1 - kb) + 1;  // <= 2 (AUG_TILE - 1) + taps + 1: the host sized the LDS for it
			for (int i = tid; i < span; i += AUG_THREADS) xs[i] = aug_sample<I16>(xrow, r.len, kb + i);
			__syncthreads();
		}
		int64_t m = nz ? (r.offset + n0 + tid) % noise_len : 0;
		for (int i = 0; i < AUG_TILE / AUG_THREADS; ++i) {
			const int64_t n = n0 + tid + i * AUG_THREADS;
			if (n < T) {
				float y = 0.f;
				if (n <= n_last) {
					if (resamp) {
						const uint64_t pos = (uint64_t)n * r.step;
						const unsigned frac = (unsigned)pos, ph = frac >> (32 - AUG_PBITS);
						const float f = (float)((frac << AUG_PBITS) >> 8) * (1.0f / 16777216.0f);  // where between phase ph and ph + 1, 24 bits: exact
						const float* xp = xs + (int)((int64_t)(pos >> 32) - H - kb);
						const float* cp = aug_lds + ph;
						float acc = 0.f;
						for (int j = 0; j < taps; ++j) {
							const float t0 = cp[j * AUG_PW], t1 = cp[j * AUG_PW + 1];
							acc = fmaf(xp[j], fmaf(f, t1 - t0, t0), acc);
						}
						y = acc;
					} else y = aug_sample<I16>(xrow, r.len, n);
					if (r.gain >= 0) y *= g;
					ex += (double)y * (double)y;
					if (nz) { const float v = nz[m]; en += (double)v * (double)v; }
				}
				orow[n] = y;
			}
			if (nz) { m += dm; if (m >= noise_len) m -= noise_len; }
		}
		if (resamp) __syncthreads();  // the span is refilled by the next tile
	}
	ex = aug_block_sum(ex, red, AUG_THREADS / 64);
	en = aug_block_sum(en, red, AUG_THREADS / 64);
	if (tid == 0) {
		double* p = partials + ((int64_t)b * AUG_PARTS + part) * 2;
		p[0] = ex; p[1] = en;
	}
}

__global__ __launch_bounds__(AUG_THREADS) void augment_mix_kernel(float* __restrict__ out, const int64_t* __restrict__ params, const float* __restrict__ noise, int64_t noise_rows, int64_t noise_len,
                                                                  const float* __restrict__ snr_table, int snr_steps, const double* __restrict__ partials, int nparts, float* __restrict__ scales, int64_t T) {
	__shared__ float s_scale;
	const int tid = threadIdx.x, b = blockIdx.y;
	const AugRow r = aug_row(params, b, T, -1, 0, noise_rows, noise_len, snr_steps);
	if (tid == 0) {
		float a = 0.f;
		if (r.noise >= 0) {
			double ex = 0.0, en = 0.0;
			for (int i = 0; i < nparts; ++i) { ex += partials[((int64_t)b * AUG_PARTS + i) * 2]; en += partials[((int64_t)b * AUG_PARTS + i) * 2 + 1]; }
			if (ex > 0.0 && en > 0.0) a = (float)((double)snr_table[r.snr] * sqrt(ex / en));
		}
		s_scale = a;
		if (blockIdx.x == 0) scales[b] = a;
	}
	__syncthreads();
	const float a = s_scale;
	const int64_t n0 = (int64_t)blockIdx.x * AUG_TILE;
	if (a == 0.f || n0 >= r.out_len) return;
	const float* nz = noise + r.noise * noise_len;
	float* orow = out + (int64_t)b * T;
	const int64_t dm = AUG_THREADS % noise_len;
	int64_t m = (r.offset + n0 + tid) % noise_len;
	for (int i = 0; i < AUG_TILE / AUG_THREADS; ++i) {
		const int64_t n = n0 + tid + i * AUG_THREADS;
		if (n < r.out_len) orow[n] = fmaf(a, nz[m], orow[n]);
		m += dm; if (m >= noise_len) m -= noise_len;
	}
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_augment_kernel(const float* __restrict__ x, const float* __restrict__ xlen, const int64_t* __restrict__ keys, const int64_t* __restrict__ epoch_p,
                                                                    uint64_t seed, int F, int T, int nf, int fw, int nt, int tw, unsigned tf_fix, int fill_mean, float fill_value,
                                                                    float* __restrict__ out, float* __restrict__ fill_out, int* __restrict__ masks_out) {
	__shared__ int m_start[2 * SPEC_MAX_MASKS], m_width[2 * SPEC_MAX_MASKS];
	__shared__ double red[SPEC_THREADS / 64];
	__shared__ float s_fill;
	const int tid = threadIdx.x, b = blockIdx.y;
	int valid = valid_len(xlen, b, T);
	valid = valid < 0 ? 0 : (valid > T ? T : valid);
	const float* xb = x + (int64_t)b * F * T;
	float* ob = out + (int64_t)b * F * T;
	if (tid < nf + nt) {
		const uint64_t key = (uint64_t)keys[b];
		const unsigned epoch = (unsigned)epoch_p[0];
		int w, s;
		if (tid < nf) {
			w = (int)aug_uint(aug_draw(seed, epoch, key, AS_FREQ_WIDTH, tid), min(fw, F));
			s = (int)aug_uint(aug_draw(seed, epoch, key, AS_FREQ_START, tid), F - w);
		} else {
			const int64_t lim = ((int64_t)valid * (int64_t)tf_fix) >> 24;  // floor(time_fraction * valid) with time_fraction in 24-bit fixed point
			w = (int)aug_uint(aug_draw(seed, epoch, key, AS_TIME_WIDTH, tid - nf), min((int64_t)tw, lim));
			s = (int)aug_uint(aug_draw(seed, epoch, key, AS_TIME_START, tid - nf), valid - w);
		}
		m_start[tid] = s; m_width[tid] = w;
		if (blockIdx.x == 0 && masks_out != nullptr) { masks_out[((int64_t)b * (nf + nt) + tid) * 2] = s; masks_out[((int64_t)b * (nf + nt) + tid) * 2 + 1] = w; }
	}
	if (fill_mean) {  // every workgroup of the utterance forms the same mean in the same order: lane-strided float64 sums, then the fixed tree
		const int64_t n_el = (int64_t)F * valid;
		double acc = 0.0;
		for (int64_t e = tid; e < n_el; e += SPEC_THREADS) { const int f = (int)(e / valid), t = (int)(e - (int64_t)f * valid); acc += (double)xb[(int64_t)f * T + t]; }
		acc = aug_block_sum(acc, red, SPEC_THREADS / 64);
		if (tid == 0) s_fill = n_el > 0 ? (float)(acc / (double)n_el) : 0.f;
	} else if (tid == 0) s_fill = fill_value;
	__syncthreads();
	const float fill = s_fill;
	if (blockIdx.x == 0 && tid == 0) fill_out[b] = fill;
	const unsigned n_all = (unsigned)F * (unsigned)T;
	for (unsigned e = blockIdx.x * SPEC_THREADS + tid; e < n_all; e += gridDim.x * SPEC_THREADS) {
		const unsigned f = e / (unsigned)T, t = e - f * (unsigned)T;
		float v = xb[e];
		if ((int)t < valid) {
			bool masked = false;
			for (int i = 0; i < nf; ++i) masked |= (f - (unsigned)m_start[i]) < (unsigned)m_width[i];
			for (int i = nf; i < nf + nt; ++i) masked |= (t - (unsigned)m_start[i]) < (unsigned)m_width[i];
			if (masked) v = fill;
		}
		ob[e] = v;
	}
}

// ------------------------------------------------------------------------------------------------ host side

extern "C" int convasr_philox(const int64_t* counters, int64_t n, uint32_t key0, uint32_t key1, int64_t* out, void* stream) {
	CONVASR_CHECK_ARG(n >= 0 && n < (1ll << 31), "philox: %lld counters outside [0, 2^31)", (long long)n);
	if (n == 0) return 0;
	CONVASR_CHECK_ARG(counters && out, "philox: NULL pointer");
	hipLaunchKernelGGL(philox_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, counters, n, key0, key1, out);
	CONVASR_CHECK_LAUNCH("philox");
	return 0;
}

extern "C" int convasr_augment_tile(void) { return AUG_TILE; }
extern "C" int convasr_augment_phases(void) { return AUG_PHASES; }
extern "C" int convasr_augment_parts(void) { return AUG_PARTS; }

static int64_t aug_lds_bytes(int taps) { return AUG_RED_DOUBLES * 8 + (taps > 0 ? ((int64_t)taps * AUG_PW + 2 * (AUG_TILE - 1) + taps + 2) * 4 : 0); }

static int aug_check_batch(const char* name, int B, int64_t T) {
	CONVASR_CHECK_ARG(B >= 0 && T >= 0, "%s: bad batch (B %d, T %lld)", name, B, (long long)T);
	if (B > 65535) return convasr_fail(CONVASR_EUNSUPPORTED, "%s: a batch of %d > 65535", name, B);
	if (T >= (1ll << 31)) return convasr_fail(CONVASR_EUNSUPPORTED, "%s: T %lld >= 2^31", name, (long long)T);
	return 0;
}

static int aug_check_noise(const char* name, const void* noise, int64_t rows, int64_t len) {
	if (noise == nullptr && rows == 0) return 0;
	CONVASR_CHECK_ARG(noise != nullptr && rows >= 1 && len >= 1, "%s: a noise bank of %lld rows x %lld samples (pointer %p)", name, (long long)rows, (long long)len, noise);
	if (rows >= (1ll << 31) || len >= (1ll << 31)) return convasr_fail(CONVASR_EUNSUPPORTED, "%s: a noise bank of %lld x %lld, 2^31 or more rows or samples", name, (long long)rows, (long long)len);
	return 0;
}

extern "C" int convasr_augment_params(const float* xlen, const int64_t* keys, const int64_t* min_out_len, int B, int64_t T, uint64_t seed, int64_t epoch, const uint64_t* steps,
                                      int n_speeds, uint32_t speed_thr, int gain_steps, uint32_t gain_thr, int64_t noise_rows, int64_t noise_len, int snr_steps, uint32_t noise_thr,
                                      int64_t* params, float* xlen_out, void* stream) {
	if (const int e = aug_check_batch("augment_params", B, T)) return e;
	CONVASR_CHECK_ARG(steps != nullptr && n_speeds >= 1, "augment_params: an empty speed table");
	if (n_speeds > AUG_MAX_SPEEDS) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_params: %d speeds > %d", n_speeds, AUG_MAX_SPEEDS);
	AugSteps st = {};
	for (int i = 0; i < n_speeds; ++i) {
		if (steps[i] < (AUG_ONE >> 1) || steps[i] > (AUG_ONE << 1)) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_params: speed %d (step %llu / 2^32) outside [0.5, 2]", i, (unsigned long long)steps[i]);
		st.v[i] = steps[i];
	}
	CONVASR_CHECK_ARG(epoch >= 0 && epoch < (1ll << 32), "augment_params: epoch %lld outside [0, 2^32)", (long long)epoch);
	CONVASR_CHECK_ARG(speed_thr <= (1u << 24) && gain_thr <= (1u << 24) && noise_thr <= (1u << 24), "augment_params: a probability threshold above 2^24");
	if (gain_steps < 0 || gain_steps > AUG_MAX_STEPS) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_params: %d gain steps outside [0, %d]", gain_steps, AUG_MAX_STEPS);
	CONVASR_CHECK_ARG(noise_rows >= 0, "augment_params: %lld noise rows", (long long)noise_rows);
	if (noise_rows > 0) {
		CONVASR_CHECK_ARG(noise_len >= 1, "augment_params: noise rows of %lld samples", (long long)noise_len);
		if (noise_rows >= (1ll << 31) || noise_len >= (1ll << 31)) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_params: a noise bank of %lld x %lld, 2^31 or more rows or samples", (long long)noise_rows, (long long)noise_len);
		if (snr_steps < 1 || snr_steps > AUG_MAX_STEPS) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_params: %d SNR steps outside [1, %d]", snr_steps, AUG_MAX_STEPS);
	}
	if (B == 0) return 0;
	CONVASR_CHECK_ARG(xlen && keys && params && xlen_out, "augment_params: NULL pointer");
	if (T == 0) return 0;
	hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)ceil_div64(B, 256)), dim3(256), 0, (hipStream_t)stream, xlen, keys, min_out_len, B, T, seed, (unsigned)epoch, st, n_speeds, speed_thr,
	                   gain_steps, gain_thr, noise_rows, noise_len, snr_steps, noise_thr, params, xlen_out);
	CONVASR_CHECK_LAUNCH("augment_params");
	return 0;
}

extern "C" int convasr_augment_waveform(const void* x, int x_dtype, int B, int64_t T, const int64_t* params, const float* table, int n_speeds, int taps, const float* gain_table, int gain_steps,
                                        const float* noise, int64_t noise_rows, int64_t noise_len, float* out, double* partials, void* stream) {
	if (const int e = aug_check_batch("augment_waveform", B, T)) return e;
	CONVASR_CHECK_ARG(x_dtype == CONVASR_I16 || x_dtype == CONVASR_F32, "augment_waveform: input dtype %d is neither CONVASR_I16 nor CONVASR_F32", x_dtype);
	CONVASR_CHECK_ARG(taps >= 0 && !(taps & 1), "augment_waveform: taps %d is not 0 or an even number >= 2", taps);
	if (n_speeds < 0 || n_speeds > AUG_MAX_SPEEDS) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_waveform: %d speeds outside [0, %d]", n_speeds, AUG_MAX_SPEEDS);
	if (aug_lds_bytes(taps) > AUG_LDS_MAX) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_waveform: %d taps x %d phases and a tile's span need %lld bytes of LDS, %d at most", taps, AUG_PW, (long long)aug_lds_bytes(taps), AUG_LDS_MAX);
	CONVASR_CHECK_ARG(taps == 0 || (table != nullptr && n_speeds >= 1), "augment_waveform: %d taps without a table", taps);
	if (gain_steps < 0 || gain_steps > AUG_MAX_STEPS) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_waveform: %d gain steps outside [0, %d]", gain_steps, AUG_MAX_STEPS);
	CONVASR_CHECK_ARG(gain_steps == 0 || gain_table != nullptr, "augment_waveform: %d gain steps without a table", gain_steps);
	if (const int e = aug_check_noise("augment_waveform", noise, noise_rows, noise_len)) return e;
	if (B == 0 || T == 0) return 0;
	CONVASR_CHECK_ARG(x && params && out && partials, "augment_waveform: NULL pointer");
	const int64_t ntiles = ceil_div64(T, AUG_TILE);
	const dim3 grid((unsigned)(ntiles < AUG_PARTS ? ntiles : AUG_PARTS), (unsigned)B);
	const size_t lds = (size_t)aug_lds_bytes(taps);
	static unsigned long long allowed_i16 = 0, allowed_f32 = 0;
#define AUG_LAUNCH(I16, MASK) do { \
		if (lds > 64 * 1024) convasr_allow_160k_lds((const void*)augment_waveform_kernel<I16>, MASK); \
		hipLaunchKernelGGL(augment_waveform_kernel<I16>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, x, params, table, n_speeds, taps, gain_table, gain_steps, noise, noise_rows, noise_len, out, partials, T, ntiles); \
	} while (0)
	if (x_dtype == CONVASR_I16) AUG_LAUNCH(true, allowed_i16); else AUG_LAUNCH(false, allowed_f32);
#undef AUG_LAUNCH
	CONVASR_CHECK_LAUNCH("augment_waveform");
	return 0;
}

extern "C" int convasr_augment_mix(float* out, int B, int64_t T, const int64_t* params, const float* noise, int64_t noise_rows, int64_t noise_len, const float* snr_table, int snr_steps,
                                   const double* partials, float* scales, void* stream) {
	if (const int e = aug_check_batch("augment_mix", B, T)) return e;
	CONVASR_CHECK_ARG(noise != nullptr, "augment_mix: no noise bank");
	if (const int e = aug_check_noise("augment_mix", noise, noise_rows, noise_len)) return e;
	if (snr_steps < 1 || snr_steps > AUG_MAX_STEPS) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_mix: %d SNR steps outside [1, %d]", snr_steps, AUG_MAX_STEPS);
	if (B == 0 || T == 0) return 0;
	CONVASR_CHECK_ARG(out && params && snr_table && partials && scales, "augment_mix: NULL pointer");
	const int64_t ntiles = ceil_div64(T, AUG_TILE);
	hipLaunchKernelGGL(augment_mix_kernel, dim3((unsigned)ntiles, (unsigned)B), dim3(AUG_THREADS), 0, (hipStream_t)stream, out, params, noise, noise_rows, noise_len, snr_table, snr_steps, partials,
	                   (int)(ntiles < AUG_PARTS ? ntiles : AUG_PARTS), scales, T);
	CONVASR_CHECK_LAUNCH("augment_mix");
	return 0;
}

extern "C" int convasr_spec_augment_tile(void) { return SPEC_THREADS; }

extern "C" int convasr_spec_augment(const float* x, const float* xlen, const int64_t* keys, const int64_t* epoch, uint64_t seed, int B, int F, int T, int freq_masks, int freq_width,
                                    int time_masks, int time_width, uint32_t time_fraction_q24, int fill_mean, float fill_value, float* out, float* fill_out, int32_t* masks_out, void* stream) {
	CONVASR_CHECK_ARG(B >= 0 && F >= 0 && T >= 0, "spec_augment: bad shape (%d, %d, %d)", B, F, T);
	if (B > 65535) return convasr_fail(CONVASR_EUNSUPPORTED, "spec_augment: a batch of %d > 65535", B);
	if ((int64_t)F * T >= (1ll << 31)) return convasr_fail(CONVASR_EUNSUPPORTED, "spec_augment: %d x %d features per utterance >= 2^31", F, T);
	if (freq_masks < 0 || freq_masks > SPEC_MAX_MASKS || time_masks < 0 || time_masks > SPEC_MAX_MASKS) return convasr_fail(CONVASR_EUNSUPPORTED, "spec_augment: %d frequency / %d time masks outside [0, %d]", freq_masks, time_masks, SPEC_MAX_MASKS);
	CONVASR_CHECK_ARG(freq_width >= 0 && time_width >= 0 && time_fraction_q24 <= (1u << 24), "spec_augment: bad widths (%d, %d) or time fraction (%u / 2^24)", freq_width, time_width, time_fraction_q24);
	if (B == 0 || F == 0 || T == 0) return 0;
	CONVASR_CHECK_ARG(x && xlen && keys && epoch && out && fill_out, "spec_augment: NULL pointer");
	CONVASR_CHECK_ARG(x != out, "spec_augment: in place");
	int64_t split = ceil_div64((int64_t)F * T, 32 * SPEC_THREADS);
	split = split < 1 ? 1 : (split > SPEC_MAX_SPLIT ? SPEC_MAX_SPLIT : split);
	hipLaunchKernelGGL(spec_augment_kernel, dim3((unsigned)split, (unsigned)B), dim3(SPEC_THREADS), 0, (hipStream_t)stream, x, xlen, keys, epoch, seed, F, T, freq_masks, freq_width, time_masks,
	                   time_width, time_fraction_q24, fill_mean, fill_value, out, fill_out, masks_out);
	CONVASR_CHECK_LAUNCH("spec_augment");
	return 0;
}
