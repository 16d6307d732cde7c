// Training-time augmentation of a collated batch on the GPU: speed perturbation, gain and noise mixing on the waveforms (convasr_augment_params,
// convasr_augment_waveform, convasr_augment_mix), room reverberation between gain and noise (convasr_augment_reverb_params,
// convasr_augment_reverb: the last section of this file) and SpecAugment on the log-mel features (convasr_spec_augment).  The rules live in
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

// ================================================================================================ room reverberation
//
// z[n] = sum_k h[k] y[n + d - k] for n < out_len, h one row of a bank of room impulse responses, d the index of its direct path: uniformly
// partitioned overlap-save convolution.  Blocks of RV_BK outputs, FFTs of RV_N = 2 RV_BK complex points in LDS, the impulse response cut into
// P = ceil(rir_len / RV_BK) parts.  With y'[n] = y[n + d] (0 outside the utterance), segment j = y'[(j - 1) RV_BK, (j + 1) RV_BK) and H_p the
// spectrum of part p behind RV_BK zeros, output block m is the upper half of IFFT(sum_p X_(m - p) H_p).  Two real blocks share one complex FFT
// WITHOUT being separated: a convolution with a real h is linear over the complex numbers, so with Mh = ceil(M / 2) of the utterance's M
// blocks, C_j = FFT(segment j + i segment (j + Mh)) gives IFFT(sum_p C_(m - p) H_p) = block m + i block (m + Mh).
//
// An utterance whose shorter operand, min(rir_len, out_len), has at most RV_DIRECT samples skips the FFTs: reverb_finish_kernel sums its at most
// RV_DIRECT products per sample directly, in ascending tap index.
//
// Three launches: reverb_spectra_kernel (one workgroup per C_j, j in [-P, Mh), and per H_p, into the workspace), reverb_apply_kernel (one
// workgroup per pair of output blocks: the P complex multiply-adds per bin in registers in ascending p, the inverse FFT, the samples) and
// reverb_finish_kernel (the zeros behind out_len, the bit-exact copy of the utterances without a row, and the two energies in the tile
// ownership and order of augment_waveform_kernel, so that augment_mix_kernel reads them unchanged).  The FFT is a radix-2 Stockham autosort
// between two LDS buffers with the caller's twiddle table; nothing depends on B or on the utterance's place.  A twiddle is TWO floats per
// component, the float64 value rounded to fp32 and the remainder: with one float |w| misses 1 by up to 3e-8, and the few twiddles of the early
// passes are used so often that a transform loses 3e-8 of its amplitude, a convolution (three transforms) 1e-7 -- more than one fp32 ulp of
// the noise scale that convasr_augment_mix derives from the energy.  The low parts enter the product's fma chain first, so they are not
// rounded away.
#define RV_BK 1024
#define RV_N (2 * RV_BK)
#define RV_THREADS 256
#define RV_PER_LANE (RV_N / RV_THREADS)
#define RV_MAX_LEN 32768
#define RV_DIRECT 32  // min(rir_len, out_len) up to here: the at most RV_DIRECT products per sample are summed directly
enum { AS_REVERB_FIRE = 12, AS_REVERB_ROW = 13 };

__global__ __launch_bounds__(256) void reverb_params_kernel(const int64_t* __restrict__ keys, int B, uint64_t seed, unsigned epoch, int64_t rows, unsigned thr, int64_t* __restrict__ rir_row) {
	const int b = blockIdx.x * 256 + threadIdx.x;
	if (b >= B) return;
	const uint64_t key = (uint64_t)keys[b];
	int64_t row = -1;
	if (aug_fires(aug_draw(seed, epoch, key, AS_REVERB_FIRE, 0), thr)) row = aug_uint(aug_draw(seed, epoch, key, AS_REVERB_ROW, 0), rows - 1);
	rir_row[b] = row;
}

// what one utterance convolves with, every field forced into the range the kernels index with; row < 0: nothing
struct RvRow { int64_t row, len, delay, out_len; int P, Mh; bool direct; };
__device__ __forceinline__ RvRow rv_row(const int64_t* __restrict__ params, const int64_t* __restrict__ rir_row, const int64_t* __restrict__ rir_len, const int64_t* __restrict__ rir_delay, int b,
                                        int64_t T, int64_t R, int64_t Lmax, int pmax) {
	RvRow r;
	r.out_len = params[(int64_t)b * AUG_PARAMS + AP_OUT_LEN];
	r.out_len = r.out_len < 0 ? 0 : (r.out_len > T ? T : r.out_len);
	r.row = rir_row[b]; r.len = 0; r.delay = 0; r.P = 0;
	if (r.row < 0 || r.row >= R) r.row = -1;
	else {
		r.len = rir_len[r.row]; r.delay = rir_delay[r.row];
		if (r.len < 1 || r.len > Lmax || r.len > (int64_t)pmax * RV_BK || r.delay < 0 || r.delay >= r.len) r.row = -1;
		else r.P = (int)((r.len + RV_BK - 1) / RV_BK);
	}
	r.Mh = (int)(((r.out_len + RV_BK - 1) / RV_BK + 1) / 2);
	r.direct = r.row >= 0 && (r.len < r.out_len ? r.len : r.out_len) <= RV_DIRECT;
	return r;
}

// RV_N points from `a` (scratch `b`), forward or inverse (unscaled): eleven radix-2 Stockham passes, every lane four butterflies per pass.
// Returns the buffer that holds the result in natural order; the caller's fill of `a` needs no barrier of its own.
__device__ __forceinline__ float2* rv_fft(float2* a, float2* b, const float4* tw, bool inverse) {
	const int tid = threadIdx.x;
	for (int ns = 1; ns < RV_N; ns <<= 1) {
		__syncthreads();
		const int shift = RV_BK / ns;  // W_(2 ns)^k = tw[k * RV_BK / ns]
#pragma unroll
		for (int q = 0; q < RV_BK / RV_THREADS; ++q) {
			const int j = tid + q * RV_THREADS, k = j & (ns - 1);
			const float4 w = tw[k * shift];  // (cos hi, -sin hi, cos lo, -sin lo)
			const float sh = inverse ? -w.y : w.y, sl = inverse ? -w.w : w.w;
			const float2 u0 = a[j], u1 = a[j + RV_BK];
			const float tx = fmaf(u1.x, w.x, fmaf(-u1.y, sh, fmaf(u1.x, w.z, -u1.y * sl))), ty = fmaf(u1.x, sh, fmaf(u1.y, w.x, fmaf(u1.x, sl, u1.y * w.z)));
			const int j0 = (j << 1) - k;
			b[j0] = make_float2(u0.x + tx, u0.y + ty);
			b[j0 + ns] = make_float2(u0.x - tx, u0.y - ty);
		}
		float2* t = a; a = b; b = t;
	}
	__syncthreads();
	return a;
}

__global__ __launch_bounds__(RV_THREADS) void reverb_spectra_kernel(const float* __restrict__ y, const int64_t* __restrict__ params, const int64_t* __restrict__ rir_row, const float* __restrict__ rir,
                                                                    const int64_t* __restrict__ rir_len, const int64_t* __restrict__ rir_delay, int64_t R, int64_t Lmax, int pmax, int mh_max,
                                                                    const float4* __restrict__ twiddles, float2* __restrict__ ws, int64_t T) {
	__shared__ float2 buf[2][RV_N];
	__shared__ float4 tw[RV_BK];
	const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.x, nsig = mh_max + pmax;
	const RvRow r = rv_row(params, rir_row, rir_len, rir_delay, b, T, R, Lmax, pmax);
	if (r.row < 0 || r.direct) return;  // (uniform over the workgroup, like the one below; out_len == 0 is direct)
	if (s < nsig ? s >= r.Mh + r.P : s - nsig >= r.P) return;
	for (int i = tid; i < RV_BK; i += RV_THREADS) tw[i] = twiddles[i];
	if (s < nsig) {  // C_j, j = s - P: segment j in the real parts, segment j + Mh in the imaginary ones
		const float* yrow = y + (int64_t)b * T;
		const int64_t n0 = ((int64_t)(s - r.P) - 1) * RV_BK + r.delay, n1 = n0 + (int64_t)r.Mh * RV_BK;
		for (int t = tid; t < RV_N; t += RV_THREADS) {
			const int64_t i0 = n0 + t, i1 = n1 + t;
			buf[0][t] = make_float2(i0 >= 0 && i0 < r.out_len ? yrow[i0] : 0.f, i1 >= 0 && i1 < r.out_len ? yrow[i1] : 0.f);
		}
	} else {  // H_p: part p of the impulse response behind RV_BK zeros
		const float* h = rir + r.row * Lmax;
		const int64_t k0 = (int64_t)(s - nsig) * RV_BK;
		for (int t = tid; t < RV_N; t += RV_THREADS) buf[0][t] = make_float2(t < RV_BK && k0 + t < r.len ? h[k0 + t] : 0.f, 0.f);
	}
	const float2* res = rv_fft(buf[0], buf[1], tw, false);
	float2* dst = ws + ((int64_t)b * (nsig + pmax) + s) * RV_N;
	for (int t = tid; t < RV_N; t += RV_THREADS) dst[t] = res[t];
}

__global__ __launch_bounds__(RV_THREADS) void reverb_apply_kernel(const int64_t* __restrict__ params, const int64_t* __restrict__ rir_row, const int64_t* __restrict__ rir_len,
                                                                  const int64_t* __restrict__ rir_delay, int64_t R, int64_t Lmax, int pmax, int mh_max, const float4* __restrict__ twiddles,
                                                                  const float2* __restrict__ ws, float* __restrict__ out, int64_t T) {
	__shared__ float2 buf[2][RV_N];
	__shared__ float4 tw[RV_BK];
	const int tid = threadIdx.x, b = blockIdx.y, m = blockIdx.x, nsig = mh_max + pmax;
	const RvRow r = rv_row(params, rir_row, rir_len, rir_delay, b, T, R, Lmax, pmax);
	if (r.row < 0 || r.direct || m >= r.Mh) return;  // (uniform over the workgroup)
	for (int i = tid; i < RV_BK; i += RV_THREADS) tw[i] = twiddles[i];
	const float2* wb = ws + (int64_t)b * (nsig + pmax) * RV_N;
	float2 acc[RV_PER_LANE];
#pragma unroll
	for (int q = 0; q < RV_PER_LANE; ++q) acc[q] = make_float2(0.f, 0.f);
	for (int p = 0; p < r.P; ++p) {  // slot of C_(m - p) = m - p + P in [1, Mh + P), slot of H_p = nsig + p: both written by reverb_spectra_kernel
		const float2* X = wb + (int64_t)(m - p + r.P) * RV_N;
		const float2* H = wb + (int64_t)(nsig + p) * RV_N;
#pragma unroll
		for (int q = 0; q < RV_PER_LANE; ++q) {
			const float2 a = X[tid + q * RV_THREADS], h = H[tid + q * RV_THREADS];
			acc[q].x = fmaf(-a.y, h.y, fmaf(a.x, h.x, acc[q].x));
			acc[q].y = fmaf(a.y, h.x, fmaf(a.x, h.y, acc[q].y));
		}
	}
#pragma unroll
	for (int q = 0; q < RV_PER_LANE; ++q) buf[0][tid + q * RV_THREADS] = acc[q];
	const float2* res = rv_fft(buf[0], buf[1], tw, true);
	float* orow = out + (int64_t)b * T;
	const int64_t n0 = (int64_t)m * RV_BK, n1 = n0 + (int64_t)r.Mh * RV_BK;
	for (int i = tid; i < RV_BK; i += RV_THREADS) {  // the upper half is free of the circular wrap; 1 / RV_N is a power of two
		const float2 v = res[RV_BK + i];
		if (n0 + i < r.out_len) orow[n0 + i] = v.x * (1.0f / RV_N);
		if (n1 + i < r.out_len) orow[n1 + i] = v.y * (1.0f / RV_N);
	}
}

__global__ __launch_bounds__(AUG_THREADS) void reverb_finish_kernel(const float* __restrict__ y, const int64_t* __restrict__ params, const int64_t* __restrict__ rir_row, const float* __restrict__ rir, const int64_t* __restrict__ rir_len,
                                                                    const int64_t* __restrict__ rir_delay, int64_t R, int64_t Lmax, int pmax, const float* __restrict__ noise, int64_t noise_rows,
                                                                    int64_t noise_len, float* __restrict__ out, double* __restrict__ partials, int64_t T, int64_t ntiles) {
	__shared__ double red[AUG_RED_DOUBLES];
	const int tid = threadIdx.x, b = blockIdx.y, part = blockIdx.x, nparts = gridDim.x;
	const AugRow r = aug_row(params, b, T, -1, 0, noise_rows, noise_len, AUG_MAX_STEPS);
	const RvRow rv = rv_row(params, rir_row, rir_len, rir_delay, b, T, R, Lmax, pmax);
	const bool copy = rv.row < 0;
	const float* h = rir + (copy ? 0 : rv.row) * Lmax;
	const float* yrow = y + (int64_t)b * T;
	float* orow = out + (int64_t)b * T;
	const float* nz = (noise != nullptr && r.noise >= 0) ? noise + r.noise * noise_len : nullptr;
	const int64_t dm = AUG_THREADS % (nz ? noise_len : 1);
	double ex = 0.0, en = 0.0;
	for (int64_t tile = part; tile < ntiles; tile += nparts) {
		const int64_t n0 = tile * AUG_TILE;
		int64_t m = nz ? (r.offset + n0 + tid) % noise_len : 0;
		for (int i = 0; i < AUG_TILE / AUG_THREADS; ++i) {
			const int64_t n = n0 + tid + i * AUG_THREADS;
			if (n < T) {
				if (n < r.out_len) {
					float z;
					if (copy) z = yrow[n];
					else if (rv.direct) {  // taps k with 0 <= n + d - k < out_len, ascending
						const int64_t k_lo = n + rv.delay - r.out_len + 1 > 0 ? n + rv.delay - r.out_len + 1 : 0, k_hi = n + rv.delay < rv.len - 1 ? n + rv.delay : rv.len - 1;
						z = 0.f;
						for (int64_t k = k_lo; k <= k_hi; ++k) z = fmaf(h[k], yrow[n + rv.delay - k], z);
					} else z = orow[n];
					if (copy || rv.direct) orow[n] = z;
					ex += (double)z * (double)z;
					if (nz) { const float v = nz[m]; en += (double)v * (double)v; }
				} else orow[n] = 0.f;
			}
			if (nz) { m += dm; if (m >= noise_len) m -= noise_len; }
		}
	}
	ex = aug_block_sum(ex, red, AUG_THREADS / 64);
	en = aug_block_sum(en, red, AUG_THREADS / 64);
	if (tid == 0) {
		double* p = partials + ((int64_t)b * AUG_PARTS + part) * 2;
		p[0] = ex; p[1] = en;
	}
}

extern "C" int convasr_augment_reverb_block(void) { return RV_BK; }
extern "C" int convasr_augment_reverb_direct(void) { return RV_DIRECT; }

static int64_t rv_parts(int64_t max_rir_len) { return ceil_div64(max_rir_len < 1 ? 1 : (max_rir_len > RV_MAX_LEN ? RV_MAX_LEN : max_rir_len), RV_BK); }
static int64_t rv_half_blocks(int64_t T) { return (ceil_div64(T, RV_BK) + 1) / 2; }

extern "C" int64_t convasr_augment_reverb_workspace_bytes(int B, int64_t T, int64_t max_rir_len) {
	if (B <= 0 || T <= 0) return 0;
	return (int64_t)B * (rv_half_blocks(T) + 2 * rv_parts(max_rir_len)) * RV_N * (int64_t)sizeof(float2);
}

extern "C" int convasr_augment_reverb_params(const int64_t* keys, int B, uint64_t seed, int64_t epoch, int64_t rir_rows, uint32_t reverb_thr, int64_t* rir_row, void* stream) {
	if (const int e = aug_check_batch("augment_reverb_params", B, 0)) return e;
	CONVASR_CHECK_ARG(epoch >= 0 && epoch < (1ll << 32), "augment_reverb_params: epoch %lld outside [0, 2^32)", (long long)epoch);
	CONVASR_CHECK_ARG(reverb_thr <= (1u << 24), "augment_reverb_params: a probability threshold above 2^24");
	CONVASR_CHECK_ARG(rir_rows >= 1, "augment_reverb_params: a bank of %lld impulse responses", (long long)rir_rows);
	if (rir_rows >= (1ll << 31)) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_reverb_params: a bank of %lld impulse responses, 2^31 or more", (long long)rir_rows);
	if (B == 0) return 0;
	CONVASR_CHECK_ARG(keys && rir_row, "augment_reverb_params: NULL pointer");
	hipLaunchKernelGGL(reverb_params_kernel, dim3((unsigned)ceil_div64(B, 256)), dim3(256), 0, (hipStream_t)stream, keys, B, seed, (unsigned)epoch, rir_rows, reverb_thr, rir_row);
	CONVASR_CHECK_LAUNCH("augment_reverb_params");
	return 0;
}

extern "C" int convasr_augment_reverb(const float* y, int B, int64_t T, const int64_t* params, const int64_t* rir_row, const float* rir, int64_t rir_rows, int64_t rir_max_len, const int64_t* rir_len,
                                      const int64_t* rir_delay, const int64_t* rir_len_host, const int64_t* rir_delay_host, const float* twiddles, const float* noise, int64_t noise_rows,
                                      int64_t noise_len, float* out, double* partials, void* workspace, int64_t workspace_bytes, void* stream) {
	if (const int e = aug_check_batch("augment_reverb", B, T)) return e;
	CONVASR_CHECK_ARG(rir != nullptr && rir_len != nullptr && rir_delay != nullptr && rir_len_host != nullptr && rir_delay_host != nullptr, "augment_reverb: NULL bank pointer");
	CONVASR_CHECK_ARG(rir_rows >= 1 && rir_max_len >= 1, "augment_reverb: a bank of %lld impulse responses x %lld taps", (long long)rir_rows, (long long)rir_max_len);
	if (rir_rows >= (1ll << 31)) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_reverb: a bank of %lld impulse responses, 2^31 or more", (long long)rir_rows);
	int64_t longest = 0;
	for (int64_t i = 0; i < rir_rows; ++i) {
		const int64_t len = rir_len_host[i], d = rir_delay_host[i];
		CONVASR_CHECK_ARG(len >= 1 && len <= rir_max_len, "augment_reverb: impulse response %lld has %lld taps, outside [1, %lld]", (long long)i, (long long)len, (long long)rir_max_len);
		if (len > RV_MAX_LEN) return convasr_fail(CONVASR_EUNSUPPORTED, "augment_reverb: impulse response %lld has %lld taps > %d", (long long)i, (long long)len, RV_MAX_LEN);
		CONVASR_CHECK_ARG(d >= 0 && d < len, "augment_reverb: impulse response %lld has its delay %lld outside [0, %lld)", (long long)i, (long long)d, (long long)len);
		longest = len > longest ? len : longest;
	}
	if (const int e = aug_check_noise("augment_reverb", noise, noise_rows, noise_len)) return e;
	if (B == 0 || T == 0) return 0;
	CONVASR_CHECK_ARG(y && params && rir_row && twiddles && out && partials, "augment_reverb: NULL pointer");
	CONVASR_CHECK_ARG(y != out, "augment_reverb: in place");
	const int64_t need = convasr_augment_reverb_workspace_bytes(B, T, longest);
	CONVASR_CHECK_ARG(workspace != nullptr && workspace_bytes >= need, "augment_reverb: a workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
	const int pmax = (int)rv_parts(longest), mh_max = (int)rv_half_blocks(T);
	const int64_t ntiles = ceil_div64(T, AUG_TILE);
	hipLaunchKernelGGL(reverb_spectra_kernel, dim3((unsigned)(mh_max + 2 * pmax), (unsigned)B), dim3(RV_THREADS), 0, (hipStream_t)stream, y, params, rir_row, rir, rir_len, rir_delay, rir_rows, rir_max_len,
	                   pmax, mh_max, (const float4*)twiddles, (float2*)workspace, T);
	CONVASR_CHECK_LAUNCH("augment_reverb (spectra)");
	hipLaunchKernelGGL(reverb_apply_kernel, dim3((unsigned)mh_max, (unsigned)B), dim3(RV_THREADS), 0, (hipStream_t)stream, params, rir_row, rir_len, rir_delay, rir_rows, rir_max_len, pmax, mh_max,
	                   (const float4*)twiddles, (const float2*)workspace, out, T);
	CONVASR_CHECK_LAUNCH("augment_reverb (apply)");
	hipLaunchKernelGGL(reverb_finish_kernel, dim3((unsigned)(ntiles < AUG_PARTS ? ntiles : AUG_PARTS), (unsigned)B), dim3(AUG_THREADS), 0, (hipStream_t)stream, y, params, rir_row, rir, rir_len, rir_delay, rir_rows,
	                   rir_max_len, pmax, noise, noise_rows, noise_len, out, partials, T, ntiles);
	CONVASR_CHECK_LAUNCH("augment_reverb (finish)");
	return 0;
}
