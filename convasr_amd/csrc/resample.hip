// audio.read_audio's decode + mono mix + audio.resample (audio.py:113-126, 150-159) in one pass on the GPU: convasr_resample.
// The reference resamples with librosa on the CPU, seconds per hour-long file; here the band-limited rational resampler is defined by this
// project (include/convasr_hip.h, unpinned against librosa): output n sits at input time n M / L, its phase (n M) mod L selects one column
// of a table of L x taps coefficients that the host computed in float64, and the sum runs over the taps in ascending input index in fp32
// with one fma per tap -- the same sequence of operations on every route, so the result does not depend on the launch geometry.
//
// Routes.  tile: a workgroup of RS_TILE threads owns RS_TILE consecutive outputs of one output channel, decodes (int16 -> float, de-interleave,
// mono mean) the input span those outputs need into LDS once and streams the coefficients -- from LDS when the whole table is small (one or
// two phases: 48 -> 16 kHz, 8 -> 16 kHz), otherwise from the table in global memory, [tap][phase] so that the 64 lanes of a wave read inside
// one row of L floats (44.1 -> 16 kHz: 160 phases x 374 taps = 239 KB, served by L2).  direct: one output per thread, every sample decoded
// from global memory as it is used -- for ratios whose span does not fit in LDS (a steep downsampling).  Nothing waits between workgroups.
#include "common.h"

#define RS_TILE 256                  // outputs per workgroup = threads per workgroup
#define RS_MAX_CHANNELS 8
#define RS_MAX_TABLE (1 << 22)       // L * taps
#define RS_MAX_SAMPLES (1ll << 40)   // T_in * C
#define RS_LDS_BYTES (64 * 1024)     // what a workgroup of the tile route may take (the default dynamic-LDS limit)
#define RS_TABLE_LDS 4096            // the table goes to LDS up to this many entries
#define RS_MAX_BLOCKS (1 << 24)      // grid.x; more tiles than that are walked in a stride loop

template <bool I16> __device__ __forceinline__ float rs_one(const void* __restrict__ x, int64_t T_in, int C, int c, int64_t k) {
	if (I16) return __fdiv_rn((float)((const int16_t*)x)[k * C + c], 32767.f);  // s2f_numpy (audio.py:15): a correctly rounded fp32 divide
	return ((const float*)x)[(int64_t)c * T_in + k];
}

// sample k of output channel ch: 0 outside [0, T_in); with mono the fp32 sum of the channels in ascending order, divided by C
template <bool I16> __device__ __forceinline__ float rs_sample(const void* __restrict__ x, int64_t T_in, int C, int ch, int mono, int64_t k) {
	if (k < 0 || k >= T_in) return 0.f;
	if (!mono) return rs_one<I16>(x, T_in, C, ch, k);
	float s = rs_one<I16>(x, T_in, C, 0, k);
	for (int c = 1; c < C; ++c) s += rs_one<I16>(x, T_in, C, c, k);
	return __fdiv_rn(s, (float)C);
}

template <bool I16> __global__ __launch_bounds__(RS_TILE) void resample_decode_kernel(const void* __restrict__ x, float* __restrict__ out, int64_t T_in, int C, int mono) {
	const int ch = blockIdx.y;
	for (int64_t k = (int64_t)blockIdx.x * RS_TILE + threadIdx.x; k < T_in; k += (int64_t)gridDim.x * RS_TILE) out[(int64_t)ch * T_in + k] = rs_sample<I16>(x, T_in, C, ch, mono, k);
}

template <bool I16, bool TAB_LDS>
__global__ __launch_bounds__(RS_TILE) void resample_tile_kernel(const void* __restrict__ x, const float* __restrict__ table, float* __restrict__ out, int64_t T_in, int64_t T_out,
                                                                 int C, int mono, int L, int M, int taps, int64_t ntiles) {
	extern __shared__ float rs_lds[];  // [TAB_LDS: taps * L coefficients][the decoded input span]
	const int tid = threadIdx.x, ch = blockIdx.y, H = taps / 2 - 1;
	float* xs = rs_lds + (TAB_LDS ? taps * L : 0);
	if (TAB_LDS)
		for (int i = tid; i < taps * L; i += RS_TILE) rs_lds[i] = table[i];  // (the barrier after the span's fill covers it)
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t n0 = tile * RS_TILE, n_last = min(n0 + RS_TILE, T_out) - 1;
		const int64_t kb = (n0 * M) / L - H;                            // first input index any output of the tile reads
		const int span = (int)((n_last * M) / L + H + 1 - kb) + 1;     // .. and how many it reads: <= the host's rs_span_max
		for (int i = tid; i < span; i += RS_TILE) xs[i] = rs_sample<I16>(x, T_in, C, ch, mono, kb + i);
		__syncthreads();
		const int64_t n = n0 + tid;
		if (n <= n_last) {
			const int64_t t = n * M, k0 = t / L;
			const int p = (int)(t - k0 * L);
			const float* xp = xs + (int)(k0 - H - kb);  // taps j = 0 .. taps-1 are inputs k0 - H + j: indices 0 .. span-1 of xs
			float acc = 0.f;
			if (TAB_LDS) {
				const float* cp = rs_lds + p;
				for (int j = 0; j < taps; ++j) acc = fmaf(xp[j], cp[j * L], acc);
			} else {
				const float* __restrict__ cp = table + p;
				for (int j = 0; j < taps; ++j) acc = fmaf(xp[j], cp[(int64_t)j * L], acc);
			}
			out[(int64_t)ch * T_out + n] = acc;
		}
		__syncthreads();
	}
}

template <bool I16>
__global__ __launch_bounds__(RS_TILE) void resample_direct_kernel(const void* __restrict__ x, const float* __restrict__ table, float* __restrict__ out, int64_t T_in, int64_t T_out,
                                                                   int C, int mono, int L, int M, int taps) {
	const int ch = blockIdx.y, H = taps / 2 - 1;
	for (int64_t n = (int64_t)blockIdx.x * RS_TILE + threadIdx.x; n < T_out; n += (int64_t)gridDim.x * RS_TILE) {
		const int64_t t = n * M, k0 = t / L;
		const float* __restrict__ cp = table + (int)(t - k0 * L);
		float acc = 0.f;
		for (int j = 0; j < taps; ++j) acc = fmaf(rs_sample<I16>(x, T_in, C, ch, mono, k0 - H + j), cp[(int64_t)j * L], acc);
		out[(int64_t)ch * T_out + n] = acc;
	}
}

static int64_t rs_gcd(int64_t a, int64_t b) { while (b) { const int64_t r = a % b; a = b; b = r; } return a; }

struct RsRatio { int L, M; };
static int rs_ratio(int sr_in, int sr_out, RsRatio* r) {
	if (sr_in <= 0 || sr_out <= 0) return convasr_fail(CONVASR_EINVAL, "resample: bad sample rates (%d -> %d)", sr_in, sr_out);
	const int g = (int)rs_gcd(sr_in, sr_out);
	r->L = sr_out / g;
	r->M = sr_in / g;
	return 0;
}

// the envelope: outside it CONVASR_EUNSUPPORTED
static int rs_check(const RsRatio& r, int taps, int C, int64_t T_in) {
	if (C <= 0 || T_in < 0) return convasr_fail(CONVASR_EINVAL, "resample: bad arguments (C %d T_in %lld)", C, (long long)T_in);
	if (C > RS_MAX_CHANNELS) return convasr_fail(CONVASR_EUNSUPPORTED, "resample: %d channels > %d", C, RS_MAX_CHANNELS);
	if (T_in >= RS_MAX_SAMPLES / C) return convasr_fail(CONVASR_EUNSUPPORTED, "resample: %lld samples x %d channels >= 2^40", (long long)T_in, C);
	if (r.L == r.M) return 0;  // decode only: no table
	if (taps < 2 || (taps & 1)) return convasr_fail(CONVASR_EINVAL, "resample: taps %d is not an even number >= 2", taps);
	if ((int64_t)r.L * taps > RS_MAX_TABLE) return convasr_fail(CONVASR_EUNSUPPORTED, "resample: a table of %d phases x %d taps > 2^22 entries", r.L, taps);
	return 0;
}

static int64_t rs_span_max(const RsRatio& r, int taps) { return ((int64_t)(RS_TILE - 1) * r.M + r.L - 1) / r.L + taps + 1; }

extern "C" int convasr_resample_tile(void) { return RS_TILE; }

extern "C" int64_t convasr_resample_out_len(int64_t T_in, int sr_in, int sr_out) {
	RsRatio r;
	if (rs_ratio(sr_in, sr_out, &r) != 0) return -1;
	if (r.L != r.M && r.L > RS_MAX_TABLE / 2) { convasr_fail(CONVASR_EUNSUPPORTED, "resample: %d -> %d has %d phases", sr_in, sr_out, r.L); return -1; }
	if (T_in < 0 || T_in >= RS_MAX_SAMPLES) { convasr_fail(CONVASR_EUNSUPPORTED, "resample: %lld samples outside [0, 2^40)", (long long)T_in); return -1; }
	return ceil_div64(T_in * r.L, r.M);
}

extern "C" int convasr_resample_taps(int sr_in, int sr_out, double zeros, double rolloff) {
	RsRatio r;
	if (const int e = rs_ratio(sr_in, sr_out, &r)) return e;
	CONVASR_CHECK_ARG(zeros >= 1.0 && zeros <= 1024.0 && rolloff > 0.0 && rolloff <= 1.0, "resample: zeros %g outside [1, 1024] or rolloff %g outside (0, 1]", zeros, rolloff);
	if (r.L == r.M) return 0;
	const double s = rolloff * (r.L < r.M ? (double)r.L / r.M : 1.0), taps = 2.0 * (double)(int64_t)(zeros / s) + 2.0;
	if (taps * r.L > (double)RS_MAX_TABLE) return convasr_fail(CONVASR_EUNSUPPORTED, "resample: %d -> %d needs a table of %d phases x %.0f taps > 2^22 entries", sr_in, sr_out, r.L, taps);
	return (int)taps;
}

extern "C" int convasr_resample(const void* x, int x_dtype, int64_t T_in, int C, int mono, const float* table, int taps, int sr_in, int sr_out, float* out, int64_t T_out,
                                int route, void* stream) {
	RsRatio r;
	if (const int e = rs_ratio(sr_in, sr_out, &r)) return e;
	CONVASR_CHECK_ARG(x_dtype == CONVASR_I16 || x_dtype == CONVASR_F32, "resample: input dtype %d is neither CONVASR_I16 (interleaved) nor CONVASR_F32 (planar)", x_dtype);
	CONVASR_CHECK_ARG(route >= 0 && route <= 2, "resample: route %d is not 0 (automatic), 1 (tile) or 2 (direct)", route);
	if (const int e = rs_check(r, taps, C, T_in)) return e;
	CONVASR_CHECK_ARG(T_out == ceil_div64(T_in * r.L, r.M), "resample: T_out %lld is not ceil(%lld x %d / %d)", (long long)T_out, (long long)T_in, r.L, r.M);
	if (T_in == 0) return 0;
	CONVASR_CHECK_ARG(x && out && (table || r.L == r.M), "resample: NULL pointer");
	hipStream_t s = (hipStream_t)stream;
	const bool i16 = x_dtype == CONVASR_I16;
	const unsigned Cout = mono ? 1u : (unsigned)C;
	const auto blocks = [](int64_t n) { const int64_t b = ceil_div64(n, RS_TILE); return (unsigned)(b < RS_MAX_BLOCKS ? b : RS_MAX_BLOCKS); };
	if (r.L == r.M) {
		if (i16) hipLaunchKernelGGL(resample_decode_kernel<true>, dim3(blocks(T_in), Cout), dim3(RS_TILE), 0, s, x, out, T_in, C, mono);
		else hipLaunchKernelGGL(resample_decode_kernel<false>, dim3(blocks(T_in), Cout), dim3(RS_TILE), 0, s, x, out, T_in, C, mono);
		CONVASR_CHECK_LAUNCH("resample (decode)");
		return 0;
	}
	const int64_t entries = (int64_t)r.L * taps, span = rs_span_max(r, taps);
	const bool tab_lds = entries <= RS_TABLE_LDS && (entries + span) * 4 <= RS_LDS_BYTES;
	const bool fits = tab_lds || span * 4 <= RS_LDS_BYTES;
	if (route == 1 && !fits) return convasr_fail(CONVASR_EUNSUPPORTED, "resample: the tile route needs %lld bytes of LDS for %d -> %d, %d at most", (long long)(span * 4), sr_in, sr_out, RS_LDS_BYTES);
	if (fits && route != 2) {
		const int64_t ntiles = ceil_div64(T_out, RS_TILE);
		const size_t lds = (size_t)(span + (tab_lds ? entries : 0)) * 4;
		const dim3 grid(blocks(T_out), Cout);
#define RS_LAUNCH(I16, TAB) hipLaunchKernelGGL((resample_tile_kernel<I16, TAB>), grid, dim3(RS_TILE), lds, s, x, table, out, T_in, T_out, C, mono, r.L, r.M, taps, ntiles)
		if (i16) { if (tab_lds) RS_LAUNCH(true, true); else RS_LAUNCH(true, false); }
		else { if (tab_lds) RS_LAUNCH(false, true); else RS_LAUNCH(false, false); }
#undef RS_LAUNCH
		CONVASR_CHECK_LAUNCH("resample (tile)");
		return 0;
	}
	if (i16) hipLaunchKernelGGL(resample_direct_kernel<true>, dim3(blocks(T_out), Cout), dim3(RS_TILE), 0, s, x, table, out, T_in, T_out, C, mono, r.L, r.M, taps);
	else hipLaunchKernelGGL(resample_direct_kernel<false>, dim3(blocks(T_out), Cout), dim3(RS_TILE), 0, s, x, table, out, T_in, T_out, C, mono, r.L, r.M, taps);
	CONVASR_CHECK_LAUNCH("resample (direct)");
	return 0;
}
