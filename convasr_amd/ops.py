"""Tensor-level wrappers over the C ABI (no autograd here; see functional.py).

Activations travel as torch tensors of LOGICAL shape (B, C, T) -- the reference's convention -- whose memory is
channels-last: strides (T*C, 1, C).  `empty_cl` allocates one, `as_cl` converts anything else with the HIP layout kernel.
PyTorch is used for allocation, streams and dtype bookkeeping only; every arithmetic op is a kernel of libconvasr_hip.so.
"""
import math
import os
import types

import ctypes

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr, dtype_code, require_cuda

HALF_DTYPES = (torch.bfloat16, torch.float16)  # the two 16-bit storage types of the MFMA path (fp32 accumulation, fp32 master weights)

ACT_CODES = dict(none = _lib.ACT_NONE, relu = _lib.ACT_RELU, hardtanh = _lib.ACT_HARDTANH, leaky_relu = _lib.ACT_LEAKY_RELU)


def act_args(nonlinearity):
	"""('relu',) / ('hardtanh', lo, hi) / ('leaky_relu', slope) -> (code, lo, hi) (reference: models.py:368)."""
	if nonlinearity is None:
		return _lib.ACT_NONE, 0.0, 0.0
	name = nonlinearity[0]
	if name == 'relu':
		return _lib.ACT_RELU, 0.0, 0.0
	if name == 'hardtanh':
		return _lib.ACT_HARDTANH, float(nonlinearity[1]), float(nonlinearity[2])
	if name == 'leaky_relu':
		return _lib.ACT_LEAKY_RELU, float(nonlinearity[1]) if len(nonlinearity) > 1 else 0.01, 0.0
	raise ValueError(f'unsupported nonlinearity {nonlinearity}')


def empty_cl(B, C, T, dtype, device):
	return torch.empty(B, T, C, dtype = dtype, device = device).permute(0, 2, 1)


def zeros_cl(B, C, T, dtype, device):
	return torch.zeros(B, T, C, dtype = dtype, device = device).permute(0, 2, 1)


def is_cl(x):
	B, C, T = x.shape
	return x.stride(1) == 1 and x.stride(2) == C and (x.stride(0) == T * C or B == 1)


def convert(x, dtype, channels_last):
	"""(B, C, T) tensor of any strides -> new tensor of `dtype`, channels-last or torch-contiguous."""
	require_cuda(x)
	B, C, T = x.shape
	out = empty_cl(B, C, T, dtype, x.device) if channels_last else torch.empty(B, C, T, dtype = dtype, device = x.device)
	call('convasr_convert_layout', ptr(x), dtype_code(x.dtype), x.stride(0), x.stride(1), x.stride(2), ptr(out), dtype_code(dtype), out.stride(0), out.stride(1), out.stride(2), B, C, T, stream_ptr())
	return out


def as_cl(x, dtype = None):
	if x.__dict__.get('_convasr_planes_only') is not None:
		raise _lib.ConvasrHipError('this tensor is the placeholder of a layer output that exists as split-operand planes only (functional.ConvBnActFunction, planes_out): its values were never written -- only the split conv the network wired behind the layer may consume it (set CONVASR_NO_PLANES_OUT=1 to get real fp32 outputs)')
	dtype = dtype or x.dtype
	if x.dtype == dtype and is_cl(x):
		return x
	return convert(x, dtype, True)


def xlen_f32(xlen, device):
	if xlen is None:
		return None
	return xlen.to(device = device, dtype = torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------ host plumbing: argument arrays, library queries, lengths, per-call workspaces

def _ptr_array(items):
	arr = (ctypes.c_void_p * max(len(items), 1))()
	for i, t in enumerate(items):
		arr[i] = None if t is None else t.data_ptr()
	return arr


def _int_array(vals):
	return (ctypes.c_int * max(len(vals), 1))(*[int(v) for v in vals])


def _float_array(vals):
	return (ctypes.c_float * max(len(vals), 1))(*[float(v) for v in vals])


_queries = {}


def _cached_query(name, *args, ask = None):
	"""The library's answer to a pure question about integer arguments (a row count, a workspace size, "is this shape inside the kernel's
	envelope?"), asked once per distinct arguments.  Unbounded: one entry per shape the process meets.  ask: what answers in place of the
	entry point itself, where that does not take the (hashable) arguments as they stand -- arrays, an out-parameter."""
	r = _queries.get((name, ) + args)
	if r is None:
		r = _queries[(name, ) + args] = (ask or getattr(_lib.load(), name))(*args)
	return r


def _query(name, *args):
	"""_cached_query of a question the library may refuse with a negative answer: that raises ConvasrHipError with the library's message at
	once and is never stored -- a later hit would report whatever convasr_last_error() holds by then."""
	r = _queries.get((name, ) + args)
	if r is None:
		r = getattr(_lib.load(), name)(*args)
		if r < 0:
			raise _lib.ConvasrHipError(f'{name} failed: {_lib.load().convasr_last_error().decode()}')
		_queries[(name, ) + args] = r
	return r


def _frame_lengths(name, lengths, B, T, dev):
	"""Frames per utterance as the decoding kernels read them: (B,) int64 on dev, contiguous; None = all T frames of every utterance."""
	lengths = torch.full((B,), T, dtype = torch.int64, device = dev) if lengths is None else torch.as_tensor(lengths).to(device = dev, dtype = torch.int64).contiguous()
	if lengths.shape != (B,):
		raise ValueError(f'{name}: lengths of shape {tuple(lengths.shape)} for a batch of {B}')
	return lengths


def _ctc_targets(targets, in_len, tgt_len, B, dev):
	"""Targets (B, S_max) -- a flat tensor of B * S_max labels is viewed so -- and the two length vectors as the CTC kernels read them:
	int64 on dev, contiguous."""
	targets, in_len, tgt_len = (t.to(device = dev, dtype = torch.int64).contiguous() for t in (targets, in_len, tgt_len))
	return (targets.view(B, -1) if targets.ndim == 1 else targets), in_len, tgt_len


def _call_workspace(nbytes, dev, cap = None, name = None, what = None):
	"""Scratch for ONE call, handed back to the allocator after it -- not ops.workspace: that cache keeps its buffers for good, and these
	run to gigabytes.  A need above cap (where the caller has one) raises, naming the entry point and the shape (`what`)."""
	if cap is not None and nbytes > cap:
		raise _lib.ConvasrHipError(f'{name}: {nbytes} bytes of workspace needed for {what}, above the cap of {cap}')
	return torch.empty(max(nbytes, 16), dtype = torch.uint8, device = dev)


# ------------------------------------------------------------------------------------------------ frontend / instance norm

def logmel(signal, xlen, window, mel_weight, mel_bias, nfft, hop, preemphasis = 0.97, normalize = True, denom_multiplier = 1.0):
	"""LogFilterBankFrontend.forward (models.py:565-597) -> channels-last (B, nmel, F) fp32.
	denom_multiplier: models.py:570's debug_short_long_records_normalize_signal_multiplier, x / ((absmax + 1e-5) * m)."""
	require_cuda(signal, window, mel_weight, mel_bias)
	assert signal.ndim == 2
	if signal.dtype not in (torch.float32, torch.int16):
		signal = signal.to(torch.float32) if signal.is_floating_point() else signal.to(torch.int16) if signal.dtype in (torch.int8, torch.uint8) else signal.to(torch.float32)
	signal = signal.contiguous()
	B, T = signal.shape
	nmel = mel_weight.shape[0]
	F = 1 + T // hop
	absmax = None
	s = stream_ptr()
	if normalize:
		absmax = torch.empty(B, dtype = torch.float32, device = signal.device)
		call('convasr_signal_absmax', ptr(signal), dtype_code(signal.dtype), B, T, ptr(absmax), s)
		if denom_multiplier != 1.0:
			# the kernel divides by (absmax + 1e-5): hand it the peak that makes that (absmax + 1e-5) * m.  A debugging knob of the reference, off by
			# default: two B-element torch launches, not on the path of any BASELINE config
			absmax.mul_(float(denom_multiplier)).add_(1e-5 * (float(denom_multiplier) - 1.0))
	out = empty_cl(B, nmel, F, torch.float32, signal.device)
	xl = xlen_f32(xlen, signal.device)
	_lib.timed('hbm:logmel_kernel', 0.0, lambda: call('convasr_logmel_fwd', ptr(signal), dtype_code(signal.dtype), ptr(absmax), ptr(xl), ptr(window), window.shape[0], ptr(mel_weight), ptr(mel_bias), ptr(out), B, T, nfft, hop, nmel, float(preemphasis), s), nbytes = float(B * T * signal.element_size() + B * F * nmel * 4))
	return out


def instnorm(x, xlen, eps, out_dtype = None, channels_last = True, pad_time_to = 1):
	"""MaskedInstanceNorm1d.forward (models.py:694-719); xlen None = legacy unmasked branch.
	pad_time_to > 1: the result has its time axis rounded up to a multiple of it, the extra frames zero (a strided conv that follows
	sees the same zeros its own padding would have supplied; see functional.fold2)."""
	require_cuda(x)
	B, C, T = x.shape
	out_dtype = out_dtype or x.dtype
	Tp = -(-T // pad_time_to) * pad_time_to
	assert Tp == T or channels_last
	out = empty_cl(B, C, Tp, out_dtype, x.device) if channels_last else torch.empty(B, C, T, dtype = out_dtype, device = x.device)
	xl = xlen_f32(xlen, x.device)
	call('convasr_instnorm_fwd', ptr(x), dtype_code(x.dtype), x.stride(0), x.stride(1), x.stride(2), ptr(out), dtype_code(out_dtype), out.stride(0), out.stride(1), out.stride(2), ptr(xl), B, C, T, Tp, float(eps), stream_ptr())  # (the kernel writes the padding frames as zeros)
	return out


def instnorm_running(x, running_mean, running_var, num_batches_tracked, momentum, training, eps, out_dtype = None, pad_time_to = 1):
	"""nn.InstanceNorm1d(track_running_stats = True).forward (models.py:711): instance statistics + running-statistics update in training mode,
	the running statistics in eval mode; channels-last result like instnorm()."""
	require_cuda(x, running_mean, running_var)
	B, C, T = x.shape
	out_dtype = out_dtype or x.dtype
	Tp = -(-T // pad_time_to) * pad_time_to
	out = empty_cl(B, C, Tp, out_dtype, x.device)
	ws = torch.empty(B, C, 2, dtype = torch.float32, device = x.device) if training else None
	call('convasr_instnorm_running_fwd', ptr(x), dtype_code(x.dtype), x.stride(0), x.stride(1), x.stride(2), ptr(out), dtype_code(out_dtype), out.stride(0), out.stride(1), out.stride(2), B, C, T, Tp, float(eps),
		ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), float(momentum), int(bool(training)), ptr(ws), stream_ptr())
	return out


def output_lengths(xlen, B, T, device):
	"""compute_output_lengths (models.py:611-614) in one launch: int64 (B,) = ceil(xlen * T) evaluated in fp32 (xlen None: T)."""
	out = torch.empty(B, dtype = torch.int64, device = device)
	call('convasr_output_lengths', ptr(xlen_f32(xlen, device)), B, T, ptr(out), stream_ptr())
	return out


# ------------------------------------------------------------------------------------------------ conv

def cout_pad(c):
	return _cached_query('convasr_conv_cout_pad', c)


def weight_layout(w):
	"""W_KMAJOR for a (Cout, Cin, K) view of tap-major memory [K][Cout][Cin] (the training arena's layout), W_REFERENCE for a
	torch-contiguous tensor, None for anything else."""
	Cout, Cin, K = w.shape
	if w.is_contiguous():
		return _lib.W_REFERENCE  # (K == 1 is both at once: the reference layout's kernels are as good)
	if w.stride(1) == 1 and w.stride(0) == Cin and (w.stride(2) == Cout * Cin or K == 1):
		return _lib.W_KMAJOR
	return None


def _fp32_with_layout(w):
	"""A parameter as the packing kernels read it: (detached fp32 tensor, its layout code) -- the parameter's own memory when it is fp32
	in one of the two layouts the kernels know (weight_layout), a contiguous fp32 copy otherwise."""
	require_cuda(w)
	w = w.detach()
	layout = weight_layout(w) if w.dtype == torch.float32 else None
	if layout is None:
		w, layout = w.float().contiguous(), _lib.W_REFERENCE
	return w, layout


def pack_weight(w, dtype, mode = None, out = None, fwd_is_current = False):
	"""(Cout, Cin, K) fp32 parameter -> packed [K][rows_pad][cols] tensor(s) for the MFMA kernels.
	mode PACK_FWD returns the forward layout, PACK_DGRAD the dgrad layout, None both (fwd, dgrad).  `out` = (fwd, dgrad)
	buffers from an earlier call are refreshed in place (stable addresses, no re-allocation per optimizer step).
	fwd_is_current: out[0] already holds the parameter's packed forward copy (the optimizer's bf16 mirror): only dgrad is rebuilt."""
	w, layout = _fp32_with_layout(w)
	Cout, Cin, K = w.shape
	fwd, dgr = out if out is not None else (None, None)
	if fwd is None:
		assert not fwd_is_current
		fwd = torch.zeros(K, cout_pad(Cout), Cin, dtype = dtype, device = w.device)
	if dgr is None and mode in (None, _lib.PACK_DGRAD):
		dgr = torch.zeros(K, cout_pad(Cin), Cout, dtype = dtype, device = w.device)
	call('convasr_pack_conv_weight', None if fwd_is_current else ptr(w), ptr(fwd), ptr(dgr) if mode in (None, _lib.PACK_DGRAD) else None, dtype_code(dtype), Cout, Cin, K, layout, stream_ptr())
	return (fwd, dgr) if mode is None else (fwd if mode == _lib.PACK_FWD else dgr)


PEAK_BF16_FLOPS, PEAK_HBM_BYTES = 2.5e15, 8.0e12  # MI355X_MICROARCH.md: dense bf16 MFMA, HBM3E


def memory_bound(flops, nbytes):
	"""Which roofline bounds a launch (for the bench's per-kernel timer only): its algorithmic bytes at 8 TB/s against its FLOPs at 2.5 PF."""
	return nbytes / PEAK_HBM_BYTES > flops / PEAK_BF16_FLOPS


def conv_out_len(Tin, K, stride, dil, pad):
	return (Tin + 2 * pad - dil * (K - 1) - 1) // stride + 1


def _conv_stats_max_rows(B, Tout):
	return _cached_query('convasr_conv_stats_max_rows', B, Tout)


class ConvStats:
	"""Per-m-tile partial sums of a conv epilogue: buf is a flat fp64 tensor with room for max_rows x 2 x C, rows is how many the
	last launch wrote.  No atomics anywhere: the finalize kernels add the rows in a fixed order."""

	def __init__(self, C, B, Tout, device):
		self.C = C
		self.max_rows = _conv_stats_max_rows(B, Tout)
		self.buf = torch.empty(self.max_rows * 2 * C, dtype = torch.float64, device = device)
		self.rows = 0

	def fits(self, C, B, Tout, device):
		return self.C == C and self.buf.device == device and self.max_rows >= _conv_stats_max_rows(B, Tout)

	def totals(self):
		out = torch.empty(2 * self.C, dtype = torch.float64, device = self.buf.device)
		call('convasr_reduce_rows', ptr(self.buf), self.rows, 2 * self.C, ptr(out), stream_ptr())
		return out


CONV_ROUTES = ('refused', 'general', 'lds_dma', 'one_tap')  # convasr_conv1d_fwd_route's answer
CONV_ROUTE_FIELDS = ('error', 'B', 'T', 'tile_rows', 'm_tiles_per_b', 'n_tiles', 'total_tiles', 'full_tiles', 'narrow_parts', 'tail128', 'x_rows', 'xi', 'aligned_x', 'stages', 'lds_bytes', 'stats_rows')


def conv_route(x_dtype, y_dtype, B, Cin, Cout, Tin, Tout, K, stride = 1, dil = 1, pad = 0, scale = False, act = _lib.ACT_NONE, xlen = False, stats = False):
	"""Which kernel conv1d (convasr_conv1d_fwd) would launch for this geometry and these optional operands under the current
	convasr_debug_set_conv_v2 state, and what the kernel would be given: dict(route = one of CONV_ROUTES, **CONV_ROUTE_FIELDS); a refused
	geometry has the route and the error code alone.  The launch's own decision code; no launch, no GPU, not cached (it follows the debug switch)."""
	out = (ctypes.c_int * 16)()
	route = _lib.load().convasr_conv1d_fwd_route(dtype_code(x_dtype), dtype_code(y_dtype), B, Cin, Cout, Tin, Tout, K, stride, dil, pad, int(bool(scale)), act, int(bool(xlen)), int(bool(stats)), out)
	plan = dict(route = CONV_ROUTES[route], error = out[0])
	if route:
		plan.update(zip(CONV_ROUTE_FIELDS, out))
	return plan


SPLITK = os.environ.get('CONVASR_NO_SPLITK') != '1'  # A/B hook: small-batch inference launches cut over the input channels


def _splitk_plan(dtype, B, Cin, Cout, Tout, K):
	"""(splits, workspace bytes) of convasr_conv1d_fwd_splitk_plan, whose byte count comes back through an out-parameter."""
	nb = ctypes.c_int64(0)
	return _lib.load().convasr_conv1d_fwd_splitk_plan(dtype, B, Cin, Cout, Tout, K, ctypes.byref(nb)), nb.value


def _conv_timer_label(v2s, flops, nbytes, same_width, one_tap = False, suffix = ''):
	"""(family, symbol class) under which the bench's per-kernel timer books a conv launch.  v2s: the LDS-DMA kernel takes it (the family name is
	a label: fp16 launches of the same kernel are booked under it too); same_width: 16-bit input AND output; one_tap: conv1x1.hip's launches."""
	if not v2s:
		return 'conv1d_igemm (other variants)', None
	if one_tap:
		return 'hbm:conv1x1_kernel (one-tap training launches)', None  # bound by bytes moved, booked under the HBM roofline
	symbol = 'v2s16' if same_width else None
	if memory_bound(flops, nbytes):
		return 'hbm:conv1d_igemm_v2s_kernel (memory-bound launches: the 38-class decoder)', symbol
	return 'conv1d_igemm_v2s_kernel<bf16>' + suffix, symbol


def _conv_label_route(x_dtype, out_dtype, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, scale, act, xlen, stats):
	"""(the LDS-DMA family takes the launch -- conv1x1.hip's kernel is booked as one of it --, the one-tap kernel takes it) for conv1d's timer
	label: the dispatcher's own answer (convasr_conv1d_fwd_route), not a copy of its conditions.  A split-K launch is booked like the unsplit one."""
	route = conv_route(x_dtype, out_dtype, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, scale, act[0], xlen, stats)['route']
	return route in ('lds_dma', 'one_tap'), route == 'one_tap'


def conv1d(x, wp, Cout, K, stride = 1, dil = 1, pad = 0, out_dtype = None, bias = None, stats = None, scale = None, shift = None, act = (_lib.ACT_NONE, 0.0, 0.0), xlen = None, Tout = None, work = None, family = None, splitk = False):
	"""x: channels-last (B, Cin, Tin); wp: packed weights.  Returns channels-last (B, Cout, Tout).
	splitk (the inference path's launches): a launch of a few tiles -- one online request is 4-16 workgroups per layer on 256 CUs -- is cut over the
	input channels (convasr_conv1d_fwd_splitk: fp32 partial tiles, added in split order by a second kernel that also runs the epilogue).
	Tout (optional): compute only the first Tout frames of the output; work: FLOPs to book for the bench's timer (the stride-2 fold).
	stats: None, a ConvStats (the production path: partial rows, consumed by bn_finalize), or a (2 Cout,) fp64 tensor that
	receives the totals (sum, sum of squares) -- a convenience for tests and tools, one extra tiny launch."""
	B, Cin, Tin = x.shape
	assert is_cl(x), 'conv1d expects a channels-last activation'
	Tout = conv_out_len(Tin, K, stride, dil, pad) if Tout is None else Tout
	out_dtype = out_dtype or x.dtype
	y = empty_cl(B, Cout, Tout, out_dtype, x.device)
	part = stats if isinstance(stats, ConvStats) or stats is None else ConvStats(Cout, B, Tout, x.device)
	rows = ctypes.c_int(0)
	launch = lambda: call('convasr_conv1d_fwd', ptr(x), ptr(wp), ptr(y), dtype_code(x.dtype), dtype_code(out_dtype), B, Cin, Cout, Tin, Tout, K, stride, dil, pad, ptr(bias), None if part is None else ptr(part.buf), ptr(scale), ptr(shift), act[0], act[1], act[2], ptr(xlen), ctypes.byref(rows) if part is not None else None, stream_ptr())
	if splitk and SPLITK and stats is None and stride == 1 and (x.dtype in HALF_DTYPES or (x.dtype == torch.float32 and out_dtype == torch.float32)) and Cout % 8 == 0:
		plan = _cached_query('convasr_conv1d_fwd_splitk_plan', dtype_code(x.dtype), B, Cin, Cout, Tout, K, ask = _splitk_plan)
		if plan[0] >= 2:
			ws = workspace(plan[1], x.device, 'splitk')
			launch = lambda: call('convasr_conv1d_fwd_splitk', ptr(x), ptr(wp), ptr(y), dtype_code(x.dtype), dtype_code(out_dtype), B, Cin, Cout, Tin, Tout, K, dil, pad, ptr(bias), ptr(scale), ptr(shift), act[0], act[1], act[2], ptr(xlen), plan[0], ptr(ws), stream_ptr())
	if _lib.timer is None:  # (the label is for the bench's per-kernel timer only: not on the path of an ordinary step)
		launch()
	else:
		# which kernel the C side picks (conv.hip: convasr_conv1d_fwd -> convasr_conv1d_v2_try)
		es, osz = x.element_size(), (2 if out_dtype in HALF_DTYPES else 4)
		flops, nbytes_ = 2.0 * B * Tout * Cout * Cin * K if work is None else work, float(B * Tin * Cin * es + K * Cout * Cin * es + B * Tout * Cout * osz)
		v2s, one_tap = _conv_label_route(x.dtype, out_dtype, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, scale is not None, act, xlen is not None, part is not None)
		kernel, symbol = _conv_timer_label(v2s, flops, nbytes_, out_dtype == x.dtype, one_tap)
		_lib.timed(family or kernel, flops, launch, nbytes = nbytes_, symbol = symbol)
	if part is not None:
		part.rows = rows.value
		if part is not stats:
			stats.copy_(part.totals())
	return y


def conv1d_dgrad_bn_reduce(dy, packed_dgrad, Cin, K, dil, pad, bn_y, bn_scale, bn_shift, bn_mean, bn_invstd, act, dropout_p, seed, offset, xlen, bn_sums, work = None, gate = None, step_key = None):
	"""dx = dgrad(dy) with pass 1 of the consumer layer's batch-norm backward fused into the epilogue (bn_sums += per-channel sums).
	Returns dx, or None when the shape is outside the fused kernel's envelope (nothing was launched)."""
	B, Cout, Tdy = dy.shape
	T = conv_out_len(Tdy, K, 1, dil, pad)
	assert is_cl(dy) and dy.dtype in HALF_DTYPES and is_cl(bn_y) and bn_y.dtype == dy.dtype and tuple(bn_y.shape) == (B, Cin, T) and isinstance(bn_sums, ConvStats) and bn_sums.fits(Cin, B, T, dy.device), (dy.shape, bn_y.shape, Cin, T)
	rows = ctypes.c_int(0)
	dx = empty_cl(B, Cin, T, dy.dtype, dy.device)
	rc = [0]
	def run():
		rc[0] = _lib.call_rc('convasr_conv1d_dgrad_bn_reduce', ptr(dy), ptr(packed_dgrad), ptr(dx), dtype_code(dy.dtype), B, Cout, Cin, Tdy, T, K, dil, pad, ptr(bn_y), ptr(bn_scale), ptr(bn_shift), ptr(bn_mean), ptr(bn_invstd), act[0], act[1], act[2], float(dropout_p), int(seed), int(offset), step_key, ptr(xlen), ptr(bn_sums.buf), ctypes.byref(rows), ptr(gate), stream_ptr())
	if _lib.timer is None:
		run()
	else:
		flops, nbytes_ = 2.0 * B * T * Cout * Cin * K if work is None else work, float(B * Tdy * Cout * 2 + K * Cout * Cin * 2 + 2 * B * T * Cin * 2)
		kernel, symbol = _conv_timer_label(Cout % 64 == 0, flops, nbytes_, True, suffix = '+bn_bwd')
		_lib.timed(kernel, flops, run, nbytes = nbytes_, symbol = symbol)
	bn_sums.rows = rows.value
	return dx if rc[0] == 0 else None


def conv1x1_grouped(xs, wps, couts, biases = None, stats = None, outs = None, accumulate = None):
	"""n one-tap convs over the same frames in one dispatch (include/convasr_hip.h, "grouped one-tap launches").  xs: channels-last
	(B, Cin_i, T) tensors of one 16-bit dtype; wps: packed weights; stats: list of ConvStats / None; outs: list of preallocated
	(B, Cout_i, T) outputs / None; accumulate: list of bools (add into outs[i]).  Returns the outputs, or None (nothing launched) when a
	problem is outside the kernel's envelope."""
	n = len(xs)
	B, _, T = xs[0].shape
	dt = xs[0].dtype
	if n == 0 or n > 12 or dt not in HALF_DTYPES or any(x.dtype != dt or x.shape[0] != B or x.shape[2] != T or not is_cl(x) or x.shape[1] % 64 for x in xs) or any(c % 128 for c in couts):
		return None
	if any(B * T * max(x.shape[1], c) * 2 >= 2 ** 31 or c * x.shape[1] * 2 >= 2 ** 31 for x, c in zip(xs, couts)):  # the kernel's 32-bit buffer offsets (csrc/conv1x1.hip): the caller launches such branches one by one
		return None
	ys = [empty_cl(B, couts[i], T, dt, xs[0].device) if outs is None or outs[i] is None else outs[i] for i in range(n)]
	rows = ctypes.c_int(0)
	cins = [x.shape[1] for x in xs]
	launch = lambda: call('convasr_conv1x1_grouped', n, _ptr_array(xs), _ptr_array(wps), _ptr_array(ys), _ptr_array(biases) if biases else None, _ptr_array([None if s_ is None else s_.buf for s_ in stats]) if stats else None,
		_int_array(cins), _int_array(couts), _int_array(accumulate) if accumulate else None, dtype_code(dt), B, T, ctypes.byref(rows), stream_ptr())
	_lib.timed('hbm:conv1x1_kernel (one-tap training launches)', 2.0 * B * T * sum(ci * co for ci, co in zip(cins, couts)), launch, nbytes = float(2 * B * T * sum(ci + co * (2 if accumulate and accumulate[i] else 1) for i, (ci, co) in enumerate(zip(cins, couts))) + 2 * sum(ci * co for ci, co in zip(cins, couts))))
	if stats:
		for s_ in stats:
			if s_ is not None:
				s_.rows = rows.value
	return ys


def wgrad1x1_grouped(xs, dys, dws, zeros = None, accumulate = None):
	"""dws[i] (Cout_i, Cin_i, 1) fp32 (+)= the one-tap weight gradient of (xs[i], dys[i]); zeros[i] (optional): a (Cout_i,) fp32 tensor set to
	zero (the branch's bias gradient).  One dispatch + one combine for all problems.  Returns False (nothing launched) outside the envelope."""
	n = len(xs)
	B, _, T = xs[0].shape
	dt = xs[0].dtype
	cins, couts = [x.shape[1] for x in xs], [dy.shape[1] for dy in dys]
	if n == 0 or n > 12 or dt not in HALF_DTYPES or any(c % 128 for c in cins + couts) or any(not is_cl(t) or t.dtype != dt or t.shape[0] != B or t.shape[2] != T for t in list(xs) + list(dys)):
		return False
	for dw, ci, co in zip(dws, cins, couts):
		assert dw.dtype == torch.float32 and tuple(dw.shape) == (co, ci, 1) and (dw.is_contiguous() or (dw.stride(0) == ci and dw.stride(1) == 1)), (dw.shape, dw.stride())
	nb = _cached_query('convasr_wgrad1x1_grouped_workspace_bytes', tuple(cins), tuple(couts), B, T, ask = lambda ci, co, B, T: _lib.load().convasr_wgrad1x1_grouped_workspace_bytes(len(ci), _int_array(ci), _int_array(co), B, T))
	ws = workspace(nb, xs[0].device, 'wgrad')
	_lib.timed('conv1d_wgrad', 2.0 * B * T * sum(ci * co for ci, co in zip(cins, couts)), lambda: call('convasr_wgrad1x1_grouped', n, _ptr_array(xs), _ptr_array(dys), _ptr_array(dws), _ptr_array(zeros) if zeros else None,
		_int_array(cins), _int_array(couts), _int_array(accumulate) if accumulate else None, ptr(ws), dtype_code(dt), B, T, stream_ptr()))
	return True


def add16(a, b, out = None):
	"""out = a + b for two 16-bit tensors of the same (channels-last) layout; in place when out is a or b."""
	assert a.dtype == b.dtype and a.dtype in HALF_DTYPES and a.shape == b.shape and a.stride() == b.stride() and a.numel() % 8 == 0
	out = torch.empty_like(a) if out is None else out
	call('convasr_add16', ptr(a), ptr(b), ptr(out), a.numel(), dtype_code(a.dtype), stream_ptr())
	return out


_workspaces = {}
_capturing = [False]  # functional.CAPTURING (the same list object, installed by functional at import)


def workspace(nbytes, device, tag = 'default'):
	"""Grow-only scratch buffer per (device, tag, current stream): kernels that share one are ordered by that stream, and a
	buffer replaced by a bigger one is released by the caching allocator in the order of the stream it was allocated on (the
	side-stream wgrad and a main-stream wgrad of the same backward never share or free each other's slabs)."""
	if _capturing[0] or (tag == 'splitk' and device.type == 'cuda' and torch.cuda.is_current_stream_capturing()):  # (the inference path is captured by its callers -- bench_infer.py, a server -- not by train.GraphedTrainStep: ask the runtime)
		return torch.empty(max(int(nbytes), 256), dtype = torch.uint8, device = device)  # inside a graph capture: from the graph's own pool, never a cached buffer a later eager step could replace
	key = (device, tag, _lib.stream_ptr() if device.type == 'cuda' else 0)  # (the current device's current stream: kernels are launched there)
	buf = _workspaces.get(key)
	if buf is None or buf.numel() < nbytes:
		buf = torch.empty(max(int(nbytes), 1 << 20), dtype = torch.uint8, device = device)
		_workspaces[key] = buf
	return buf


def fold2_geometry(K, pad):
	"""(K', P') of the stride-1 conv over the (T / 2, 2 Cin) view that equals a stride-2 conv (K, pad); include/convasr_hip.h."""
	kf, pf = ctypes.c_int(0), ctypes.c_int(0)
	call('convasr_fold2_geometry', K, pad, ctypes.byref(kf), ctypes.byref(pf))
	return kf.value, pf.value


def fold2_pack_weight(w, dtype, pad, out = None):
	"""(Cout, Cin, K) fp32 parameter -> packed forward operand [K'][cout_pad][2 Cin] of the folded conv (refreshed in place if given)."""
	w, layout = _fp32_with_layout(w)
	Cout, Cin, K = w.shape
	if out is None:
		out = torch.empty(fold2_geometry(K, pad)[0], cout_pad(Cout), 2 * Cin, dtype = dtype, device = w.device)
	call('convasr_fold2_pack_weight', ptr(w), layout, ptr(out), dtype_code(dtype), Cout, Cin, K, pad, stream_ptr())
	return out


def fold2_unfold_wgrad(dwf, dw, pad, accumulate = False):
	"""dw (Cout, Cin, K) fp32 (+)= the folded conv's gradient dwf [K'][Cout][2 Cin]."""
	Cout, Cin, K = dw.shape
	layout = weight_layout(dw)
	assert layout is not None and dw.dtype == torch.float32 and dwf.dtype == torch.float32 and dwf.is_contiguous() and tuple(dwf.shape) == (fold2_geometry(K, pad)[0], Cout, 2 * Cin)
	call('convasr_fold2_unfold_wgrad', ptr(dwf), ptr(dw), layout, Cout, Cin, K, pad, int(accumulate), stream_ptr())
	return dw


# ------------------------------------------------------------------------------------------------ split-operand ("x3") convs

SPLIT_INPUT, SPLIT_GRAD = 0, 1  # plane orders of split3(): (hi, lo, hi) for a conv input, (hi, hi, lo) for an output gradient


def split3(x, dtype, order):
	"""fp32 channels-last (B, C, T) -> its three 16-bit planes per frame, memory [B][T][3][C] (include/convasr_hip.h, "split-operand
	convs"), returned as the channels-last (B, 3 C, T) tensor the forward / dgrad kernels read; split3_frames() is the weight gradient's view."""
	B, C, T = x.shape
	assert is_cl(x) and x.dtype == torch.float32 and dtype in HALF_DTYPES and C % 8 == 0
	out = empty_cl(B, 3 * C, T, dtype, x.device)
	_lib.timed('hbm:split3_kernel', 0.0, lambda: call('convasr_split3', ptr(x), ptr(out), dtype_code(dtype), B * T, C, int(order), stream_ptr()), nbytes = float(B * T * C * 10))
	return out


def split3_frames(x3):
	"""The (B, 3 C, T) plane tensor of split3() read as (B, C, 3 T): frame 3 t + p = plane p of frame t (the same memory)."""
	B, C3, T = x3.shape
	assert is_cl(x3) and C3 % 3 == 0
	return x3.as_strided((B, C3 // 3, 3 * T), (T * C3, 1, C3 // 3))


def split3_plane(x3, plane = 0):
	"""One plane of a (B, 3 C, T) plane tensor as a dense channels-last (B, C, T) tensor (a strided copy)."""
	B, C3, T = x3.shape
	C = C3 // 3
	assert is_cl(x3) and C3 % 3 == 0
	out = empty_cl(B, C, T, x3.dtype, x3.device)
	out.permute(0, 2, 1).copy_(x3.as_strided((B, T, C), (T * C3, C3, 1), x3.storage_offset() + plane * C))
	return out


def conv1d_wgrad_hi(x3, dy, Cout, K, dil, pad, dw, accumulate = False, work = None, family = None):
	"""conv1d_wgrad (stride 1) of plane 0 (hi) of the split-operand plane tensor x3 (B, 3 Cin, Tin) against a dense 16-bit dy: the plane is read in
	place (frames 3 Cin elements apart, convasr_conv1d_wgrad_ld) inside the LDS-DMA kernel's envelope, copied out first outside it."""
	B, C3, Tin = x3.shape
	Cin, Tout = C3 // 3, dy.shape[2]
	layout = weight_layout(dw)
	assert is_cl(x3) and is_cl(dy) and x3.dtype == dy.dtype and x3.dtype in HALF_DTYPES and layout is not None and dw.dtype == torch.float32 and tuple(dw.shape) == (Cout, Cin, K), (dw.shape, dw.stride())
	if not _cached_query('convasr_conv1d_wgrad_ld_supported', dtype_code(x3.dtype), B, Cin, Cout, Tin, Tout, K, dil, C3, Cout):  # outside the LDS-DMA kernel's envelope (channel counts not multiples of 128, a tap window too wide for its LDS ring): a dense copy of the plane
		return conv1d_wgrad(split3_plane(x3), dy, Cout, K, 1, dil, pad, dw, accumulate = accumulate, work = work, family = family)
	return _wgrad_launch(dw, layout, (B, Cin, Cout, Tin, Tout, K, 1, dil), work, family, lambda ws, layout: call('convasr_conv1d_wgrad_ld', ptr(x3), C3, ptr(dy), Cout, ptr(dw), ptr(ws), dtype_code(dy.dtype), B, Cin, Cout, Tin, Tout, K, dil, pad, int(accumulate), layout, stream_ptr()))


def pack_weight_split3(w, dtype, out = None, want_dgrad = True, dgrad_planes = 3):
	"""(Cout, Cin, K) fp32 parameter -> (fwd [K][cout_pad][3 Cin], dgrad [K][cin_pad][3 Cout]) split operands, refreshed in place when
	`out` = (fwd, dgrad) of an earlier call.  want_dgrad = False: the forward planes only (dgrad is returned as None).  dgrad_planes = 1: the
	dgrad operand as the ordinary 16-bit one, [K][cin_pad][Cout] (w_hi alone: a one-product backward)."""
	w, layout = _fp32_with_layout(w)
	Cout, Cin, K = w.shape
	fwd, dgr = out if out is not None else (None, None)
	if fwd is None:
		fwd = torch.zeros(K, cout_pad(Cout), 3 * Cin, dtype = dtype, device = w.device)
	if dgr is None and want_dgrad:
		dgr = torch.zeros(K, cout_pad(Cin), dgrad_planes * Cout, dtype = dtype, device = w.device)
	assert dgr is None or dgr.shape[2] == dgrad_planes * Cout
	call('convasr_pack_conv_weight_split3', ptr(w), layout, ptr(fwd), ptr(dgr) if want_dgrad else None, dgrad_planes, dtype_code(dtype), Cout, Cin, K, stream_ptr())
	return fwd, (dgr if want_dgrad else None)


def colsum(y, out, accumulate = False):
	"""out (C,) fp32 (+)= sum over (b, t) of a channels-last (B, C, T) tensor: a conv's bias gradient on its own."""
	B, C, T = y.shape
	assert is_cl(y) and out.dtype == torch.float32 and out.numel() == C and out.is_contiguous()
	ws = workspace(_cached_query('convasr_colsum_workspace_bytes', B * T, C), y.device, 'colsum')
	call('convasr_colsum', ptr(y), dtype_code(y.dtype), B * T, C, ptr(out), ptr(ws), int(accumulate), stream_ptr())
	return out


def _wgrad_launch(dw, layout, geometry, work, family, launch):
	"""What the weight-gradient launches share: the layout override for one tap, the split-K workspace of the geometry
	(B, Cin, Cout, Tin, Tout, K, stride, dil) and the timed launch(ws, layout).  Returns dw."""
	B, Cin, Cout, Tin, Tout, K, stride, dil = geometry
	if K == 1 and (Cout * Cin) % 4 == 0:
		layout = _lib.W_KMAJOR  # one tap: the two layouts are the same memory, and the tap-major combine is the streaming one
	ws = workspace(_cached_query('convasr_conv1d_wgrad_workspace_bytes', *geometry), dw.device, 'wgrad')
	_lib.timed(family or 'conv1d_wgrad', 2.0 * B * Tout * Cout * Cin * K if work is None else work, lambda: launch(ws, layout))
	return dw


def conv1d_wgrad(x, dy, Cout, K, stride, dil, pad, dw, dbias = None, accumulate = False, work = None, family = None):
	"""dw (Cout, Cin, K) fp32 (+)= wgrad; x, dy channels-last of the same dtype.  dw is torch-contiguous (the reference's layout) or a
	view of tap-major memory (weight_layout: the training arena's gradients)."""
	B, Cin, Tin = x.shape
	Tout = dy.shape[2]
	layout = weight_layout(dw)
	assert is_cl(x) and is_cl(dy) and x.dtype == dy.dtype and layout is not None and dw.dtype == torch.float32 and tuple(dw.shape) == (Cout, Cin, K), (dw.shape, dw.stride())
	return _wgrad_launch(dw, layout, (B, Cin, Cout, Tin, Tout, K, stride, dil), work, family, lambda ws, layout: call('convasr_conv1d_wgrad', ptr(x), ptr(dy), ptr(dw), ptr(dbias), ptr(ws), dtype_code(x.dtype), B, Cin, Cout, Tin, Tout, K, stride, dil, pad, int(accumulate), layout, stream_ptr()))


WGRAD_ROUTES = ('refused', 'general', 'lds_dma')  # convasr_conv1d_wgrad_plan's answer


def wgrad_plan(dtype, B, Cin, Cout, Tin, Tout, K, stride = 1, dil = 1, x_ld = 0, dy_ld = 0):
	"""Which kernel conv1d_wgrad (or, with pitches x_ld / dy_ld, convasr_conv1d_wgrad_ld) would launch for this geometry under the current
	convasr_debug_set_conv_v2 state, and its plan: dict(route = one of WGRAD_ROUTES, splits, chunks_per_split, chunks_per_b, tap_groups, x_rows);
	a refused geometry has the route alone.  No launch, no GPU, and not cached (the answer follows the debug switch): the tests ask it so
	that their shapes follow the library's cost model, like scan_tile()."""
	out = (ctypes.c_int * 5)()
	route = _lib.load().convasr_conv1d_wgrad_plan(dtype_code(dtype), B, Cin, Cout, Tin, Tout, K, stride, dil, x_ld, dy_ld, out)
	plan = dict(route = WGRAD_ROUTES[route])
	if route:
		plan.update(zip(('splits', 'chunks_per_split', 'chunks_per_b', 'tap_groups', 'x_rows'), out))
	return plan


def wgrad1x1_grouped_plan(dtype, cins, couts, B, T):
	"""(splits, chunks_per_split) common to the problems of a wgrad1x1_grouped launch, or None where it would be refused.  No launch, no GPU."""
	out = (ctypes.c_int * 2)()
	ok = _lib.load().convasr_wgrad1x1_grouped_plan(len(cins), _int_array(cins), _int_array(couts), dtype_code(dtype), B, T, out)
	return (out[0], out[1]) if ok else None


# ------------------------------------------------------------------------------------------------ grouped conv (the separable block's first half)

def grouped_conv1d(x, w, bias, groups, stride = 1, pad = 0, relu = True):
	"""nn.Conv1d(Cin, Cout, K, groups = G) + bias (+ ReLU) on a channels-last activation; w: fp32 (Cout, Cin / G, K) of any strides."""
	B, Cin, Tin = x.shape
	Cout, cgi, K = w.shape
	assert is_cl(x) and w.dtype == torch.float32 and cgi * groups == Cin
	Tout = conv_out_len(Tin, K, stride, 1, pad)
	y = empty_cl(B, Cout, Tout, x.dtype, x.device)
	call('convasr_grouped_conv1d_fwd', ptr(x), ptr(w), w.stride(0), w.stride(1), w.stride(2), ptr(bias), ptr(y), dtype_code(x.dtype), B, Cin, Cout, Tin, Tout, K, stride, pad, groups, int(relu), stream_ptr())
	return y


def grouped_conv1d_dgrad(dy, y_act, w, Cin, Tin, groups, stride = 1, pad = 0):
	B, Cout, Tout = dy.shape
	K = w.shape[2]
	assert is_cl(dy) and (y_act is None or (is_cl(y_act) and y_act.dtype == dy.dtype))
	dx = empty_cl(B, Cin, Tin, dy.dtype, dy.device)
	call('convasr_grouped_conv1d_dgrad', ptr(dy), ptr(y_act), ptr(w), w.stride(0), w.stride(1), w.stride(2), ptr(dx), dtype_code(dy.dtype), B, Cin, Cout, Tin, Tout, K, stride, pad, groups, stream_ptr())
	return dx


def grouped_conv1d_wgrad(x, dy, y_act, dw, dbias, groups, stride = 1, pad = 0, accumulate = False):
	B, Cin, Tin = x.shape
	Cout, Tout, K = dy.shape[1], dy.shape[2], dw.shape[2]
	assert is_cl(x) and is_cl(dy) and dw.dtype == torch.float32 and tuple(dw.shape) == (Cout, Cin // groups, K)
	ws = workspace(_cached_query('convasr_grouped_conv1d_wgrad_workspace_bytes', B, Cin, Cout, K, groups), x.device, 'grouped_wgrad')
	call('convasr_grouped_conv1d_wgrad', ptr(x), ptr(dy), ptr(y_act), ptr(dw), dw.stride(0), dw.stride(1), dw.stride(2), ptr(dbias), ptr(ws), dtype_code(x.dtype), B, Cin, Cout, Tin, Tout, K, stride, pad, groups, int(accumulate), stream_ptr())
	return dw


# ------------------------------------------------------------------------------------------------ batch norm + activation

def bn_finalize(stats, n, gamma, beta, running_mean, running_var, momentum, eps, num_batches_tracked = None):
	"""stats: a ConvStats (partial rows of the conv launch) or a (2 C,) fp64 tensor of totals."""
	if isinstance(stats, ConvStats):
		buf, rows, C = stats.buf, stats.rows, stats.C
	else:
		buf, rows, C = stats, 1, stats.numel() // 2
	out = torch.empty(4, C, dtype = torch.float32, device = buf.device)  # mean, invstd, scale, shift
	o = out.data_ptr()
	call('convasr_bn_finalize', ptr(buf), rows, n, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(momentum), float(eps), o, o + 4 * C, o + 8 * C, o + 12 * C, C, ptr(num_batches_tracked), stream_ptr())
	return out


def bn_finalize_grouped(stats, n, gammas, betas, running_means, running_vars, momenta, epss, num_batches_tracked):
	"""bn_finalize for several batch norms of one channel count in one launch; stats: ConvStats of equal row counts.  Returns one (4, C)
	fp32 tensor per batch norm (mean, invstd, scale, shift)."""
	k, C, rows = len(stats), stats[0].C, stats[0].rows
	assert all(s_.C == C and s_.rows == rows for s_ in stats)
	out = torch.empty(k, 4, C, dtype = torch.float32, device = stats[0].buf.device)
	call('convasr_bn_finalize_grouped', k, _ptr_array([s_.buf for s_ in stats]), rows, n, _ptr_array(gammas), _ptr_array(betas), _ptr_array(running_means), _ptr_array(running_vars),
		_float_array(momenta), _float_array(epss), _ptr_array([out[i] for i in range(k)]), _ptr_array(num_batches_tracked), C, stream_ptr())
	return [out[i] for i in range(k)]


def bn_bwd_finalize_grouped(sums, gammas, means, invstds, n, coefs, dgammas, dbetas, accumulate):
	"""bn_bwd_finalize for several batch norms in one launch; sums: (2 C,) fp64 totals each."""
	k, C = len(sums), sums[0].numel() // 2
	call('convasr_bn_bwd_finalize_grouped', k, _ptr_array(sums), _int_array([1] * k), _ptr_array(gammas), _ptr_array(means), _ptr_array(invstds), _ptr_array(coefs), _ptr_array(dgammas), _ptr_array(dbetas),
		_int_array(accumulate), int(n), C, stream_ptr())


def bn_bwd_reduce_many(dz, gate, dropout_p, ys, means, invstds, gammas, coefs, dgammas, dbetas, accumulate):
	"""Pass 1 of a dense block's backward in one sweep from the stored gates (include/convasr_hip.h): returns g; fills coefs / dgammas / dbetas."""
	B, C, T = dz.shape
	assert is_cl(dz) and dz.dtype in HALF_DTYPES and all(is_cl(y) and y.dtype == dz.dtype and y.shape == dz.shape for y in ys) and gate.dtype == torch.uint8 and gate.numel() * 8 == dz.numel()
	g = empty_cl(B, C, T, dz.dtype, dz.device)
	k = len(ys)
	ws = workspace(_cached_query('convasr_bn_bwd_reduce_many_workspace_bytes', k, B, T, C), dz.device, 'bn_bwd')
	_lib.timed('hbm:bn_act_bwd_reduce_kernel', 0.0, lambda: call('convasr_bn_bwd_reduce_many', ptr(dz), ptr(gate), float(dropout_p), ptr(g), k, _ptr_array(ys), _ptr_array(means), _ptr_array(invstds), _ptr_array(gammas),
		_ptr_array(coefs), _ptr_array(dgammas), _ptr_array(dbetas), _int_array(accumulate), ptr(ws), dtype_code(dz.dtype), B, T, C, stream_ptr()), nbytes = float(B * T * C * dz.element_size() * (2 + k)))
	return g


def bn_bwd_apply_grouped(g, ys, coefs):
	"""dy_i = A_i g + B_i y_i + D_i for every (y_i, coef_i), g read once.  Returns the list of dy_i."""
	B, C, T = g.shape
	assert is_cl(g) and g.dtype in HALF_DTYPES and all(is_cl(y) and y.dtype == g.dtype and y.shape == g.shape for y in ys)
	dys = [empty_cl(B, C, T, g.dtype, g.device) for _ in ys]
	_lib.timed('hbm:bn_act_bwd_apply_kernel', 0.0, lambda: call('convasr_bn_bwd_apply_grouped', ptr(g), len(ys), _ptr_array(ys), _ptr_array(coefs), _ptr_array(dys), dtype_code(g.dtype), B, T, C, stream_ptr()), nbytes = float(B * T * C * g.element_size() * (1 + 2 * len(ys))))
	return dys


def bn_eval_scale_shift(gamma, beta, running_mean, running_var, eps):
	C = running_mean.numel()
	out = torch.empty(2, C, dtype = torch.float32, device = running_mean.device)
	call('convasr_bn_eval_scale_shift', ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(eps), ptr(out[0]), ptr(out[1]), C, stream_ptr())
	return out


def bn_act(y, scale, shift, act, xlen = None, res = (), rscale = (), rshift = (), dropout_p = 0.0, seed = 0, offset = 0, out = None, gate = None, step_key = None, planes = None):
	"""gate (optional uint8 (B*T*C/8,)): receives one bit per element, set iff the gradient passes it (include/convasr_hip.h).
	step_key (optional, here and in the backward passes): device address (int) of the per-step dropout key word (functional.begin_step).
	planes (a 16-bit dtype; fp32 y with scale / shift and a clamp-type activation): the result is returned as its split-operand planes, the
	(B, 3 C, T) tensor split3(z, planes, SPLIT_INPUT) would produce, written by this pass itself."""
	B, C, T = y.shape
	assert gate is None or (gate.dtype == torch.uint8 and gate.numel() * 8 == B * C * T and gate.is_contiguous())
	assert is_cl(y) and all(is_cl(r) and r.dtype == y.dtype for r in res)
	# the two forms share one signature: (entry point, result, its dtype, bytes moved per element for the bench's timer)
	if planes is not None:
		assert y.dtype == torch.float32 and planes in HALF_DTYPES and out is None and scale is not None and act[0] != _lib.ACT_LEAKY_RELU
		entry, z, zdtype, per_elem = 'convasr_bn_act_fwd_split3', empty_cl(B, 3 * C, T, planes, y.device), planes, 10 + 4 * len(res)
	else:
		entry, z, zdtype, per_elem = 'convasr_bn_act_fwd', out if out is not None else empty_cl(B, C, T, y.dtype, y.device), y.dtype, y.element_size() * (2 + len(res))
	_lib.timed('hbm:bn_act_fwd_kernel', 0.0, lambda: call(entry, ptr(y), ptr(z), dtype_code(zdtype), ptr(scale), ptr(shift), len(res), _ptr_array(res), _ptr_array(rscale) if rscale else None, _ptr_array(rshift) if rshift else None, act[0], act[1], act[2], float(dropout_p), int(seed), int(offset), step_key, ptr(xlen), B, T, C, ptr(gate), stream_ptr()), nbytes = float(B * T * C * per_elem))
	return z


def bn_act_bwd_reduce(dz, y, scale, shift, mean, invstd, act, xlen = None, res = (), rscale = (), rshift = (), rmean = (), rinvstd = (), rsums = (), dropout_p = 0.0, seed = 0, offset = 0, sums = None, write_g = True, gamma = None, coef = None, dgamma = None, dbeta = None, accumulate = False, gate = None, step_key = None):
	"""gate: the forward pass's one-bit gradient gates (bn_act(..., gate = ...)); needs write_g = False and no residuals."""
	B, C, T = y.shape
	assert is_cl(y) and is_cl(dz) and dz.dtype == y.dtype and (gate is None or (not write_g and not res))
	g = empty_cl(B, C, T, y.dtype, y.device) if write_g else None
	ws = workspace(_cached_query('convasr_bn_bwd_workspace_bytes', B, T, C), y.device, 'bn_bwd')
	_lib.timed('hbm:bn_act_bwd_reduce_kernel', 0.0, lambda: call('convasr_bn_act_bwd_reduce', ptr(dz), ptr(y), ptr(g), dtype_code(y.dtype), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), len(res), _ptr_array(res), _ptr_array(rscale) if rscale else None, _ptr_array(rshift) if rshift else None, _ptr_array(rmean) if rmean else None, _ptr_array(rinvstd) if rinvstd else None, _ptr_array(rsums) if rsums else None, act[0], act[1], act[2], float(dropout_p), int(seed), int(offset), step_key, ptr(xlen), ptr(sums), ptr(ws), ptr(gamma), ptr(coef), ptr(dgamma), ptr(dbeta), int(accumulate), B, T, C, ptr(gate), stream_ptr()), nbytes = float(B * T * C * y.element_size() * (2 + len(res) + (1 if write_g else 0))))
	return g


def bn_act_bwd_apply(dz_or_g, y, coef, from_dz, scale = None, shift = None, act = (_lib.ACT_NONE, 0.0, 0.0), xlen = None, dropout_p = 0.0, seed = 0, offset = 0, out = None, gate = None, step_key = None, planes = None, hi_only = False):
	"""planes (a 16-bit dtype, fp32 inputs only): dy is returned as its split-operand planes, the (B, 3 C, T) tensor split3(dy, planes, SPLIT_GRAD)
	would produce -- written by this pass itself; hi_only: as the dense (B, C, T) tensor of that type instead (dy rounded once: the operand of a
	one-product backward)."""
	B, C, T = y.shape
	# the three forms share one signature: (entry point, result, its dtype, bytes moved per element for the bench's timer)
	if planes is not None:
		assert y.dtype == torch.float32 and planes in HALF_DTYPES and out is None
		if hi_only:
			entry, dy, dydtype, per_elem = 'convasr_bn_act_bwd_apply_to_half', empty_cl(B, C, T, planes, y.device), planes, 10
		else:
			entry, dy, dydtype, per_elem = 'convasr_bn_act_bwd_apply_split3', empty_cl(B, 3 * C, T, planes, y.device), planes, 14
	else:
		entry, dy, dydtype, per_elem = 'convasr_bn_act_bwd_apply', out if out is not None else empty_cl(B, C, T, y.dtype, y.device), y.dtype, y.element_size() * 3
	_lib.timed('hbm:bn_act_bwd_apply_kernel', 0.0, lambda: call(entry, ptr(dz_or_g), ptr(y), ptr(dy), dtype_code(dydtype), ptr(coef), int(from_dz), ptr(scale), ptr(shift), act[0], act[1], act[2], float(dropout_p), int(seed), int(offset), step_key, ptr(xlen), B, T, C, ptr(gate), stream_ptr()), nbytes = float(B * T * C * per_elem))
	return dy


def bn_bwd_apply(g, y, gamma, mean, invstd, sums, dgamma = None, dbeta = None, accumulate = False, need_dy = True, inplace = True):
	B, C, T = y.shape
	dy = (g if inplace else empty_cl(B, C, T, y.dtype, y.device)) if need_dy else None
	call('convasr_bn_bwd_apply', ptr(g), ptr(y), ptr(dy), dtype_code(y.dtype), ptr(gamma), ptr(mean), ptr(invstd), ptr(sums), ptr(dgamma), ptr(dbeta), int(accumulate), B, T, C, stream_ptr())
	return dy


def bn_bwd_finalize(sums, gamma, mean, invstd, n, coef = None, dgamma = None, dbeta = None, accumulate = False):
	"""sums: the ConvStats the fused dgrad epilogue filled (partial rows of sum g, sum g*xhat), or a (2 C,) fp64 tensor of totals."""
	buf, rows, C = (sums.buf, sums.rows, sums.C) if isinstance(sums, ConvStats) else (sums, 1, sums.numel() // 2)
	call('convasr_bn_bwd_finalize', ptr(buf), rows, ptr(gamma), ptr(mean), ptr(invstd), ptr(coef), ptr(dgamma), ptr(dbeta), int(accumulate), int(n), C, stream_ptr())


# ------------------------------------------------------------------------------------------------ head

def log_softmax(logits):
	"""channels-last fp32 (B, C, T) -> same."""
	B, C, T = logits.shape
	assert is_cl(logits) and logits.dtype == torch.float32
	out = empty_cl(B, C, T, torch.float32, logits.device)
	call('convasr_log_softmax_fwd', ptr(logits), ptr(out), B * T, C, stream_ptr())
	return out


def log_softmax_bwd(grad_lp, log_probs):
	B, C, T = log_probs.shape
	grad_lp = as_cl(grad_lp, torch.float32)
	out = empty_cl(B, C, T, torch.float32, log_probs.device)
	call('convasr_log_softmax_bwd', ptr(grad_lp), ptr(log_probs), ptr(out), B * T, C, stream_ptr())
	return out


def scale_rows(grad, gscale, gdiv = None):
	"""out[b] = grad[b] * gscale[b] (/ gdiv[b] if given: an int64 (B,) vector, possibly a strided column); gscale None: grad[b] / gdiv[b]."""
	B = grad.shape[0]
	out = torch.empty_like(grad)  # preserves strides (channels-last stays channels-last)
	assert gdiv is None or (gdiv.dtype == torch.int64 and gdiv.ndim == 1 and gdiv.shape[0] == B and gdiv.device == grad.device)
	call('convasr_scale_rows', ptr(grad), None if gscale is None else ptr(gscale.to(torch.float32).contiguous()), ptr(gdiv), 0 if gdiv is None else gdiv.stride(0), ptr(out), B, grad.numel() // B, stream_ptr())
	return out


def loss_head(loss_vec, ylen_col, ent = None, accumulate_iterations = 1, need_grad = True, loss_scaler = None, metric_scale = 1.0):
	"""train.py:754-756 + the gate of 769 in one launch.  Returns (out3 = [loss, loss_cur, entropy] fp32, grad_loss_vec (B,) or None,
	skipped: 1-element bool).  loss_scaler: the current state of a dynamic loss scaler (fp16 training): grad_loss_vec is scaled by it;
	metric_scale: factor on the two logged means (1 / world size ahead of a SUM all-reduce)."""
	require_cuda(loss_vec)
	B = loss_vec.shape[0]
	lv = loss_vec.detach().to(torch.float32).contiguous()
	assert ylen_col.dtype == torch.int64 and ylen_col.ndim == 1 and ylen_col.shape[0] == B and ylen_col.device == lv.device
	out3 = torch.empty(3, dtype = torch.float32, device = lv.device)
	gvec = torch.empty(B, dtype = torch.float32, device = lv.device) if need_grad else None
	skipped = torch.empty(1, dtype = torch.bool, device = lv.device)
	ent = None if ent is None else ent.detach().to(torch.float32).contiguous()
	call('convasr_loss_head', ptr(lv), ptr(ylen_col), ylen_col.stride(0), ptr(ent), B, float(accumulate_iterations), ptr(out3), ptr(gvec), ptr(skipped), ptr(loss_scaler), float(metric_scale), stream_ptr())
	return out3, gvec, skipped


def entropy(log_probs, olen = None, eps = 1e-9):
	B, C, T = log_probs.shape
	lp = as_cl(log_probs, torch.float32)
	ent = torch.empty(B, dtype = torch.float32, device = lp.device)
	ol = None if olen is None else olen.to(device = lp.device, dtype = torch.int64).contiguous()
	call('convasr_entropy', ptr(lp), ptr(ol), ptr(ent), B, T, C, float(eps), stream_ptr())
	return ent


def weighted_mean_entropy(log_probs, olen = None, eps = 1e-9, eps_id = -1):
	B, C, T = log_probs.shape
	lp = as_cl(log_probs, torch.float32)
	out = torch.empty(B, dtype = torch.float32, device = lp.device)
	ol = None if olen is None else olen.to(device = lp.device, dtype = torch.int64).contiguous()
	call('convasr_weighted_mean_entropy', ptr(lp), ptr(ol), ptr(out), B, T, C, int(eps_id) % C, float(eps), stream_ptr())
	return out


def normalize_signal(signal, eps = 1e-5, denom_multiplier = 1.0):
	"""models.py:684-686 as a standalone op: per-utterance peak (absmax kernel), then one scaling pass."""
	require_cuda(signal)
	assert signal.ndim == 2
	if signal.numel() == 0:
		return signal
	signal = signal.contiguous() if signal.dtype in (torch.float32, torch.int16) else signal.float().contiguous()
	B, T = signal.shape
	absmax = torch.empty(B, dtype = torch.float32, device = signal.device)
	call('convasr_signal_absmax', ptr(signal), dtype_code(signal.dtype), B, T, ptr(absmax), stream_ptr())
	x = signal if signal.dtype == torch.float32 else signal.float()
	out = torch.empty_like(x)
	scale = ((absmax + eps) * denom_multiplier).reciprocal()
	call('convasr_scale_rows', ptr(x), ptr(scale), None, 0, ptr(out), B, T, stream_ptr())
	return out


def argmax(log_probs):
	B, C, T = log_probs.shape
	lp = as_cl(log_probs, torch.float32)
	idx = torch.empty(B, T, dtype = torch.int64, device = lp.device)
	call('convasr_argmax', ptr(lp), ptr(idx), B * T, C, stream_ptr())
	return idx


def frame_uncertainty_row_classes():
	"""Classes up to which convasr_frame_uncertainty maps one thread to a frame; above it one wave (tests straddle it)."""
	return _cached_query('convasr_frame_uncertainty_row_classes')


def frame_uncertainty(log_probs, eps_id = -1, lengths = None):
	"""Per-frame statistics of (B, C, T) log-probs in one read (include/convasr_hip.h: convasr_frame_uncertainty has the rule).  Returns a
	namespace of (B, T) device tensors: idx int64 (ops.argmax's output, bit for bit, on every frame), and fp32 p1 (the largest probability),
	margin (p1 minus the second largest: models.margin), entropy, entropy_nb (the entropy without the class eps_id, renormalised) and p_eps
	(the probability of eps_id) -- 0 at the frames t >= lengths[b], NaN at a frame that holds a NaN.  Outside the envelope it raises
	ConvasrHipError."""
	require_cuda(log_probs)
	if log_probs.ndim != 3:
		raise ValueError(f'frame_uncertainty: (B, C, T) log-probs expected, got shape {tuple(log_probs.shape)}')
	B, C, T = log_probs.shape
	lp = as_cl(log_probs, torch.float32)
	dev = lp.device
	lengths = None if lengths is None else _frame_lengths('frame_uncertainty', lengths, B, T, dev)
	if not -C <= int(eps_id) < C:
		raise _lib.ConvasrHipError(f'frame_uncertainty: eps_id {eps_id} for {C} classes')
	idx = torch.empty(B, T, dtype = torch.int64, device = dev)
	p1, margin, ent, ent_nb, p_eps = torch.empty(5, B, T, dtype = torch.float32, device = dev).unbind(0)
	call('convasr_frame_uncertainty', ptr(lp), ptr(lengths), ptr(idx), ptr(p1), ptr(margin), ptr(ent), ptr(ent_nb), ptr(p_eps), B, T, C, int(eps_id) % C, stream_ptr())
	return types.SimpleNamespace(idx = idx, p1 = p1, margin = margin, entropy = ent, entropy_nb = ent_nb, p_eps = p_eps)


INDEX_CODES = {torch.uint8: _lib.INDEX_U8, torch.int16: _lib.INDEX_I16, torch.int32: _lib.INDEX_I32}  # include/convasr_hip.h: CONVASR_INDEX_*


def topk_frames_max_k():
	"""The largest k of topk_frames / distill_kl (CONVASR_TOPK_MAX_K)."""
	return _cached_query('convasr_topk_frames_max_k')


def _topk_dtypes(name, values_dtype, indices_dtype):
	if values_dtype not in (torch.float32, torch.float16):
		raise _lib.ConvasrHipError(f'{name}: values are float32 or float16, not {values_dtype}')
	if indices_dtype not in INDEX_CODES:
		raise _lib.ConvasrHipError(f'{name}: indices are uint8, int16 or int32, not {indices_dtype}')
	return dtype_code(values_dtype), INDEX_CODES[indices_dtype]


def topk_frames(logits, k, values_dtype = torch.float32, indices_dtype = torch.int32):
	"""The k largest logits of every frame of (B, C, T) logits and their classes, in descending order, in one read (include/convasr_hip.h:
	convasr_topk_frames has the order: larger first, ties to the lower class, a NaN above every number).  Returns (values, indices) of logical
	shape (B, k, T) -- permuted views of (B, T, k) memory, as the logits are of (B, T, C).  values_dtype float32 or float16 (the bits of
	.to(torch.float16)), indices_dtype uint8 (up to 256 classes), int16 or int32.  Outside the envelope it raises ConvasrHipError."""
	require_cuda(logits)
	if logits.ndim != 3:
		raise ValueError(f'topk_frames: (B, C, T) logits expected, got shape {tuple(logits.shape)}')
	B, C, T = logits.shape
	vcode, icode = _topk_dtypes('topk_frames', values_dtype, indices_dtype)
	lg = as_cl(logits, torch.float32)
	k = int(k)
	values = torch.empty(B, T, max(k, 0), dtype = values_dtype, device = lg.device)
	indices = torch.empty(B, T, max(k, 0), dtype = indices_dtype, device = lg.device)
	call('convasr_topk_frames', ptr(lg), ptr(values), vcode, ptr(indices), icode, B, T, C, k, stream_ptr())
	return values.permute(0, 2, 1), indices.permute(0, 2, 1)


def distill_kl(logits, values, indices, lengths, temperature = 1.0, need_grad = True, per_frame = False):
	"""tau^2 KL(truncated teacher || student) per utterance, with its gradient, in one pass over the student's (B, C, T) logits
	(include/convasr_hip.h: convasr_distill_kl has the rule).  values / indices: the teacher's k kept logits of every frame and their classes,
	logical shape (B, k, T) as topk_frames returns them (float32 or float16; uint8, int16 or int32 -- int64 indices are narrowed to int32 on
	the way in); lengths (B,): the student's frames per utterance.  Returns (kd (B,) fp32, grad (B, C, T) channels-last fp32 or None[,
	kd_frames (B, T)]): grad = d kd[b] / d logits, exactly 0 past the lengths.  Outside the envelope it raises ConvasrHipError."""
	require_cuda(logits, values, indices)
	if logits.ndim != 3 or values.ndim != 3 or values.shape != indices.shape or values.shape[0] != logits.shape[0] or values.shape[2] != logits.shape[2]:
		raise ValueError(f'distill_kl: (B, C, T) logits and (B, k, T) teacher values and indices expected, got {tuple(logits.shape)}, {tuple(values.shape)}, {tuple(indices.shape)}')
	B, C, T = logits.shape
	k = values.shape[1]
	lg = as_cl(logits, torch.float32)
	dev = lg.device
	if values.dtype not in (torch.float32, torch.float16):
		values = values.to(torch.float32)
	if indices.dtype == torch.int64:
		indices = indices.to(torch.int32)
	vcode, icode = _topk_dtypes('distill_kl', values.dtype, indices.dtype)
	values, indices = (t.to(dev).permute(0, 2, 1).contiguous() for t in (values, indices))  # (B, T, k) memory: no copy for topk_frames' own views
	lengths = _frame_lengths('distill_kl', lengths, B, T, dev)
	kd = torch.empty(B, dtype = torch.float32, device = dev)
	frames = torch.empty(B, T, dtype = torch.float32, device = dev)
	grad = empty_cl(B, C, T, torch.float32, dev) if need_grad else None
	call('convasr_distill_kl', ptr(lg), ptr(values), vcode, ptr(indices), icode, ptr(lengths), ptr(kd), ptr(frames), ptr(grad), B, T, C, k, float(temperature), stream_ptr())
	return (kd, grad, frames) if per_frame else (kd, grad)


def span_uncertainty(log_probs, stats, utt, begin, end, first = None, tokens = None, frames = None, path = None, eps = 1e-9, frame_map = None):
	"""Statistics of N spans (words) over frame_uncertainty's arrays (include/convasr_hip.h: convasr_span_uncertainty has the rule).
	log_probs (B, C, T) and stats = frame_uncertainty(log_probs, ...); utt, begin, end (N,): the utterance and the first and last position
	(inclusive) of every span.  Events: first (N + 1,), tokens and frames (first[-1],) -- ops.ctc_greedy_segments' packed tokens, frames and
	seg_first plus the total; path (B, Tp) int64 tells the inserted spaces from the asserted ones.  frame_map (B, Tp) int64: positions are
	those of another grid (a transcript) and position p of utterance b stands for frame frame_map[b, p].  Returns a namespace of (N,) device
	tensors: entropy, uncertainty and, with events, n_events int32, confidence, confidence_min, margin (None without).  Outside the
	envelope it raises ConvasrHipError."""
	require_cuda(log_probs)
	if log_probs.ndim != 3:
		raise ValueError(f'span_uncertainty: (B, C, T) log-probs expected, got shape {tuple(log_probs.shape)}')
	B, C, T = log_probs.shape
	lp = as_cl(log_probs, torch.float32)
	dev = lp.device
	for name in ('idx', 'p1', 'margin', 'entropy', 'p_eps'):
		t = getattr(stats, name)
		if tuple(t.shape) != (B, T) or t.device != dev or not t.is_contiguous():
			raise ValueError(f'span_uncertainty: stats.{name} must be a contiguous (B, T) = ({B}, {T}) tensor on {dev}')
	put = lambda t, dtype: None if t is None else torch.as_tensor(t).to(device = dev, dtype = dtype).contiguous()
	utt, begin, end = put(utt, torch.int64), put(begin, torch.int32), put(end, torch.int32)
	N = utt.numel()
	if utt.ndim != 1 or begin.shape != utt.shape or end.shape != utt.shape:
		raise ValueError(f'span_uncertainty: utt, begin and end must be (N,) tensors, got {tuple(utt.shape)}, {tuple(begin.shape)}, {tuple(end.shape)}')
	given = [t is not None for t in (first, tokens, frames)]
	if any(given) and not all(given):
		raise ValueError('span_uncertainty: first, tokens and frames come together')
	first, tokens, frames, path, frame_map = put(first, torch.int64), put(tokens, torch.int64), put(frames, torch.int32), put(path, torch.int64), put(frame_map, torch.int64)
	n_events = 0
	if all(given):
		n_events = tokens.numel()
		if first.shape != (N + 1,) or tokens.ndim != 1 or frames.shape != tokens.shape:
			raise ValueError(f'span_uncertainty: first of {N + 1} entries and tokens, frames of one length expected, got {tuple(first.shape)}, {tuple(tokens.shape)}, {tuple(frames.shape)}')
	Tp = T
	for name, t in (('path', path), ('frame_map', frame_map)):
		if t is not None:
			if t.ndim != 2 or t.shape[0] != B or (frame_map is None and t.shape[1] != T) or (frame_map is not None and t.shape[1] != frame_map.shape[1]):
				raise ValueError(f'span_uncertainty: {name} of shape {tuple(t.shape)} for {B} utterances of {T} frames')
			Tp = t.shape[1]
	ent, unc = torch.empty(2, max(N, 1), dtype = torch.float32, device = dev).unbind(0)
	n_out = conf = conf_min = margin = None
	if all(given):
		n_out = torch.empty(max(N, 1), dtype = torch.int32, device = dev)
		conf, conf_min, margin = torch.empty(3, max(N, 1), dtype = torch.float32, device = dev).unbind(0)
	call('convasr_span_uncertainty', ptr(lp), ptr(stats.idx), ptr(stats.p1), ptr(stats.margin), ptr(stats.entropy), ptr(stats.p_eps), ptr(utt), ptr(begin), ptr(end),
	     ptr(first), ptr(tokens), ptr(frames), n_events, ptr(path), ptr(frame_map), Tp, ptr(n_out), ptr(conf), ptr(conf_min), ptr(margin), ptr(ent), ptr(unc),
	     N, B, T, C, float(eps), stream_ptr())
	return types.SimpleNamespace(n_events = n_out, confidence = conf, confidence_min = conf_min, margin = margin, entropy = ent, uncertainty = unc)


# ------------------------------------------------------------------------------------------------ CTC loss

def ctc_loss(log_probs, targets, olen, ylen, blank, need_grad = True):
	"""log_probs channels-last fp32 (B, C, T); returns (nll (B,), grad channels-last (B, C, T) or None)."""
	B, C, T = log_probs.shape
	assert is_cl(log_probs) and log_probs.dtype == torch.float32
	dev = log_probs.device
	S_max = targets.numel() // B if targets.ndim == 1 else targets.shape[1]
	if not _cached_query('convasr_ctc_loss_supported', B, T, C, S_max):  # more than 1,023 labels, or more frames than the one-workgroup kernel's LDS slots hold: the tiled kernel
		return ctc_loss_long(log_probs, targets, olen, ylen, blank, need_grad = need_grad)
	targets, olen, ylen = _ctc_targets(targets, olen, ylen, B, dev)
	ws = workspace(_cached_query('convasr_ctc_workspace_bytes', B, T, S_max), dev, 'ctc')  # (never refused here: convasr_ctc_loss_supported is false for every S_max this query refuses)
	nll = torch.empty(B, dtype = torch.float32, device = dev)
	grad = empty_cl(B, C, T, torch.float32, dev) if need_grad else None
	call('convasr_ctc_loss', ptr(log_probs), ptr(targets), ptr(olen), ptr(ylen), ptr(nll), ptr(grad), ptr(ws), B, T, C, S_max, blank, stream_ptr())
	return nll, grad


def star_ctc_tiles():
	"""(states per wave, frames per renormalisation block, largest state count) of convasr_star_ctc_loss (tests straddle them)."""
	return _cached_query('convasr_star_ctc_states_per_wave'), _cached_query('convasr_star_ctc_renorm_frames'), _cached_query('convasr_star_ctc_max_states')


def star_ctc_loss(log_probs, targets, olen, ylen, blank, star_mask, star_penalty, star_enter, need_grad = True):
	"""CTC over partial transcripts (include/convasr_hip.h: convasr_star_ctc_loss has the rule): log_probs channels-last fp32 (B, C, T),
	star_mask (B, S_max + 1) bool -- gap g, before label g, may hold a star -- star_penalty / star_enter <= 0 in natural log.  Returns
	(nll (B,), grad channels-last (B, C, T) or None, star_frames (B, S_max + 1) fp32).  A shape outside the kernel's envelope raises
	ConvasrHipError: there is no fall-back to the plain loss."""
	require_cuda(log_probs)
	B, C, T = log_probs.shape
	assert is_cl(log_probs) and log_probs.dtype == torch.float32
	dev = log_probs.device
	targets, olen, ylen = _ctc_targets(targets, olen, ylen, B, dev)
	S_max = targets.shape[1]
	if star_mask.shape != (B, S_max + 1) or star_mask.dtype != torch.bool:
		raise ValueError(f'star_ctc_loss: a bool star_mask of shape {(B, S_max + 1)} expected, got {star_mask.dtype} {tuple(star_mask.shape)}')
	star_mask = star_mask.to(device = dev).contiguous()
	ws = workspace(_query('convasr_star_ctc_workspace_bytes', B, T, C, S_max), dev, 'star_ctc')
	nll = torch.empty(B, dtype = torch.float32, device = dev)
	frames = torch.empty(B, S_max + 1, dtype = torch.float32, device = dev)
	grad = empty_cl(B, C, T, torch.float32, dev) if need_grad else None
	call('convasr_star_ctc_loss', ptr(log_probs), ptr(targets), ptr(olen), ptr(ylen), ptr(star_mask), float(star_penalty), float(star_enter), ptr(nll), ptr(grad), ptr(frames), ptr(ws),
	     B, T, C, S_max, int(blank), stream_ptr())
	return nll, grad, frames


MWER_WORKSPACE_CAP = 8 << 30  # bytes of workspace one convasr_mwer_loss call may take (two lattices per hypothesis); a resource bound, not a measurement


def mwer_tiles():
	"""(states per wave, frames per renormalisation block, most labels of a hypothesis, most hypotheses of an utterance) of
	convasr_mwer_loss (tests straddle them)."""
	return _cached_query('convasr_mwer_states_per_wave'), _cached_query('convasr_mwer_renorm_frames'), _cached_query('convasr_mwer_max_labels'), _cached_query('convasr_mwer_max_hyps')


def mwer_loss(log_probs, hyps, hyp_lengths, olen, risk, blank, scale = 1.0, need_grad = True):
	"""N-best MWER loss (include/convasr_hip.h: convasr_mwer_loss has the rule; this project's own, unpinned against any outside
	implementation): log_probs channels-last fp32 (B, C, T); hyps (B, N, L_max) int64 collapsed label sequences with hyp_lengths (B, N)
	(< 0: the hypothesis is absent); risk (B, N) errors of every hypothesis; scale > 0.  Returns (loss (B,) = E[risk] - mean risk, grad
	channels-last (B, C, T) or None, hyp_nll (B, N), hyp_posterior (B, N)).  A shape outside the kernel's envelope, or one whose workspace
	is above MWER_WORKSPACE_CAP, raises ConvasrHipError: there is no composed fall-back."""
	require_cuda(log_probs)
	B, C, T = log_probs.shape
	assert is_cl(log_probs) and log_probs.dtype == torch.float32
	dev = log_probs.device
	if hyps.ndim != 3 or hyps.shape[0] != B or hyps.dtype != torch.int64:
		raise ValueError(f'mwer_loss: int64 hyps of shape (B = {B}, N, L_max) expected, got {hyps.dtype} {tuple(hyps.shape)}')
	N, L_max = hyps.shape[1:]
	if tuple(hyp_lengths.shape) != (B, N) or tuple(risk.shape) != (B, N):
		raise ValueError(f'mwer_loss: hyp_lengths and risk of shape {(B, N)} expected, got {tuple(hyp_lengths.shape)}, {tuple(risk.shape)}')
	if tuple(olen.shape) != (B,):
		raise ValueError(f'mwer_loss: olen of shape {tuple(olen.shape)} for a batch of {B}')
	if not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and 0 < scale < float('inf')):
		raise ValueError(f'mwer_loss: scale must be a finite number > 0, got {scale!r}')
	hyps, hyp_lengths, olen = (t.to(device = dev, dtype = torch.int64).contiguous() for t in (hyps, hyp_lengths, olen))
	risk = risk.to(device = dev, dtype = torch.float32).contiguous()
	nbytes = _query('convasr_mwer_workspace_bytes', B, N, T, C, L_max)
	ws = _call_workspace(nbytes, dev, MWER_WORKSPACE_CAP, 'mwer_loss', f'B {B}, N {N}, T {T}, L_max {L_max}')
	loss = torch.empty(B, dtype = torch.float32, device = dev)
	hyp_nll = torch.empty(B, N, dtype = torch.float32, device = dev)
	post = torch.empty(B, N, dtype = torch.float32, device = dev)
	grad = empty_cl(B, C, T, torch.float32, dev) if need_grad else None
	call('convasr_mwer_loss', ptr(log_probs), ptr(hyps) if L_max else None, ptr(hyp_lengths), ptr(olen), ptr(risk), float(scale), ptr(loss), ptr(grad), ptr(hyp_nll), ptr(post), ptr(ws),
	     B, N, T, C, L_max, int(blank), stream_ptr())
	return loss, grad, hyp_nll, post


CTC_LONG_WORKSPACE_CAP = 16 << 30 # bytes of workspace one convasr_ctc_loss_long call may take; a resource bound like ALIGN_LONG_WORKSPACE_CAP, not a measurement


def ctc_loss_long_tiles():
	"""(states per block, default frames per chunk) of convasr_ctc_loss_long's tiles (tests straddle them)."""
	return _cached_query('convasr_ctc_loss_long_states_per_block'), _cached_query('convasr_ctc_loss_long_chunk_frames')


def ctc_loss_long(log_probs, targets, olen, ylen, blank, need_grad = True, chunk_frames = 0, workspace_cap = CTC_LONG_WORKSPACE_CAP):
	"""ctc_loss for whole recordings (include/convasr_hip.h: convasr_ctc_loss_long): up to 131,071 labels and 2^20 frames, the same tensors in
	and out as ctc_loss, which sends here every shape its own kernel refuses.  chunk_frames: 0 = the default tile length, 16 .. 4096 forces
	it (the result does not depend on it).  The workspace (two whole fp32 lattices: about 4.4 GB for ten minutes) is allocated for this call
	and goes back to the allocator; a need above workspace_cap raises ConvasrHipError.  Not under stream capture."""
	require_cuda(log_probs)
	B, C, T = log_probs.shape
	assert is_cl(log_probs) and log_probs.dtype == torch.float32
	dev = log_probs.device
	if _capturing[0] or torch.cuda.is_current_stream_capturing():
		raise _lib.ConvasrHipError(f'ctc_loss_long: B {B}, T {T} is beyond the one-workgroup CTC kernel, and the tiled kernel (hundreds of launches over a workspace allocated per call) cannot be captured into a graph: run this step eagerly')
	targets, olen, ylen = _ctc_targets(targets, olen, ylen, B, dev)
	S_max = targets.shape[1]
	nbytes = _query('convasr_ctc_loss_long_workspace_bytes', B, T, C, S_max)
	ws = _call_workspace(nbytes, dev, workspace_cap, 'ctc_loss_long', f'B {B}, T {T}, S_max {S_max}')
	nll = torch.empty(B, dtype = torch.float32, device = dev)
	grad = empty_cl(B, C, T, torch.float32, dev) if need_grad else None
	call('convasr_ctc_loss_long', ptr(log_probs), ptr(targets), ptr(olen), ptr(ylen), ptr(nll), ptr(grad), ptr(ws), nbytes, B, T, C, S_max, int(blank), int(chunk_frames), stream_ptr())
	return nll, grad


# ------------------------------------------------------------------------------------------------ optimizer

def sumsq(flat_grad, out = None, norm_out = None, norm_scale = 1.0, loss_scaler = None):
	"""out[0] = sum of squares (fp64); norm_out (1-element fp32, optional) = sqrt(out) * norm_scale (/ the loss scaler's scale)."""
	out = out if out is not None else torch.empty(1, dtype = torch.float64, device = flat_grad.device)
	ws = workspace(_cached_query('convasr_sumsq_workspace_bytes'), flat_grad.device, 'sumsq')
	call('convasr_sumsq', ptr(flat_grad), flat_grad.numel(), ptr(out), ptr(ws), ptr(norm_out), float(norm_scale), ptr(loss_scaler), stream_ptr())
	return out


def _scaler_pair(scaler):
	"""(state read by this step, state written by it) of a dynamic loss scaler, or (None, None)."""
	if scaler is None:
		return None, None
	s_in, s_out = scaler
	assert s_in.dtype == s_out.dtype == torch.float32 and s_in.numel() == s_out.numel() == _lib.LOSS_SCALER_FLOATS and s_in.data_ptr() != s_out.data_ptr()
	return s_in, s_out


def sgd_step(p, g, buf, n, sumsq_buf, max_norm, lr, momentum, weight_decay, nesterov, first, grad_out = None, loss_gate = None, grad_scale = 1.0, p16 = None, scaler = None, lr_dev = None):
	"""lr_dev: optional 1-element fp32 device tensor that replaces `lr` when the kernel runs (captured step graphs); p16: optional 16-bit mirror of the parameters (bf16 or fp16, n elements); scaler: optional (state_in, state_out) of a dynamic loss scaler."""
	assert loss_gate is None or (loss_gate.dtype == torch.float32 and loss_gate.numel() == 1)
	assert p16 is None or (p16.dtype in HALF_DTYPES and p16.numel() == n)
	s_in, s_out = _scaler_pair(scaler)
	call('convasr_sgd_step', ptr(p), ptr(g), ptr(buf), ptr(grad_out), n, ptr(sumsq_buf), float(max_norm), float(lr), float(momentum), float(weight_decay), int(nesterov), int(first), ptr(loss_gate), float(grad_scale), ptr(p16), _lib.BF16 if p16 is None else dtype_code(p16.dtype), ptr(s_in), ptr(s_out), ptr(lr_dev), stream_ptr())


def adamw_step(p, g, exp_avg, exp_avg_sq, n, sumsq_buf, max_norm, lr, beta1, beta2, eps, weight_decay, step_in, step_out, loss_gate = None, grad_scale = 1.0, p16 = None, scaler = None, lr_dev = None):
	"""One fused torch.optim.AdamW step (+ clip_grad_norm_) over the flat arena; step_in / step_out: 1-element fp32 device tensors (applied-step counter)."""
	assert loss_gate is None or (loss_gate.dtype == torch.float32 and loss_gate.numel() == 1)
	assert p16 is None or (p16.dtype in HALF_DTYPES and p16.numel() == n)
	assert step_in.dtype == step_out.dtype == torch.float32 and step_in.data_ptr() != step_out.data_ptr()
	s_in, s_out = _scaler_pair(scaler)
	call('convasr_adamw_step', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_avg_sq), n, ptr(sumsq_buf), float(max_norm), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), ptr(step_in), ptr(step_out), ptr(loss_gate), float(grad_scale), ptr(p16), _lib.BF16 if p16 is None else dtype_code(p16.dtype), ptr(s_in), ptr(s_out), ptr(lr_dev), stream_ptr())


def ema_update(w, e, decay, k_in, k_out, e16 = None, loss_gate = None, scaler_state = None):
	"""e += (1 - d) (w - e) over two fp32 arenas, d = min(decay, (1 + k) / (10 + k)) with k = k_in[0] read on the device (k == 0: e = w); k_out[0] = k + 1.
	e16: optional 16-bit mirror of e (bf16 or fp16), rewritten with it; loss_gate: the optimizer step's gate; scaler_state: the loss scaler's state
	AFTER that step -- a non-finite gate or a recorded overflow leaves e, e16 and the counter as they were (include/convasr_hip.h has the rule)."""
	require_cuda(w, e, k_in, k_out, e16, loss_gate, scaler_state)
	assert w.dtype == e.dtype == torch.float32 and w.is_contiguous() and e.is_contiguous() and w.numel() == e.numel()
	assert k_in.dtype == k_out.dtype == torch.float32 and k_in.numel() == k_out.numel() == 1 and k_in.data_ptr() != k_out.data_ptr()
	assert e16 is None or (e16.dtype in HALF_DTYPES and e16.is_contiguous() and e16.numel() == e.numel())
	assert loss_gate is None or (loss_gate.dtype == torch.float32 and loss_gate.numel() == 1)
	assert scaler_state is None or (scaler_state.dtype == torch.float32 and scaler_state.is_contiguous() and scaler_state.numel() == _lib.LOSS_SCALER_FLOATS)
	call('convasr_ema_update', ptr(w), ptr(e), ptr(e16), _lib.BF16 if e16 is None else dtype_code(e16.dtype), e.numel(), float(decay), ptr(k_in), ptr(k_out), ptr(loss_gate), ptr(scaler_state), stream_ptr())


def swap_(a, b):
	"""Exchange the contents of two device buffers of equal size and dtype in place (one launch; the addresses do not move)."""
	require_cuda(a, b)
	assert a.dtype == b.dtype and a.numel() == b.numel() and a.is_contiguous() and b.is_contiguous()
	call('convasr_swap', ptr(a), ptr(b), a.numel() * a.element_size(), stream_ptr())


def novograd_work_table(offsets_host, device):
	"""Static work table of the fused NovoGrad step: every tensor (segment of the arena) cut into items of bounded size.
	Returns (items (n_items, 3) int64, seg_first (n_seg + 1,) int64, item_part (n_items,) fp64 scratch), all on `device`."""
	item = _lib.load().convasr_novograd_item_elems()
	items, seg_first = [], [0]
	for s_, (lo, hi) in enumerate(zip(offsets_host[:-1], offsets_host[1:])):
		for b in range(lo, max(hi, lo + 1), item):
			items.append((s_, b, min(hi, b + item)))
		seg_first.append(len(items))
	return (torch.tensor(items, dtype = torch.int64, device = device), torch.tensor(seg_first, dtype = torch.int64, device = device), torch.empty(len(items), dtype = torch.float64, device = device))


def novograd_step(p, g, mom, ema_in, ema_out, g2, offsets, n, table, max_norm, lr, beta1, beta2, eps, weight_decay, dampening, first, loss_gate = None, total_norm = None, grad_scale = 1.0, p16 = None, scaler = None, lr_dev = None):
	"""One fused NovoGrad step (+ clip_grad_norm_) over the flat arena; offsets: device int64 [n_seg + 1]; table: novograd_work_table(...)."""
	items, seg_first, item_part = table
	assert offsets.dtype == torch.int64 and ema_in.data_ptr() != ema_out.data_ptr() and g2.dtype == torch.float64
	n_seg = offsets.numel() - 1
	s_in, s_out = _scaler_pair(scaler)
	assert p16 is None or (p16.dtype in HALF_DTYPES and p16.numel() == n)
	assert int(first) >= 0 or (ema_in.numel() == n_seg + 1 and ema_out.numel() == n_seg + 1), 'first = -1 (device-side first-step detection) needs the applied-step counter behind the EMAs'
	call('convasr_novograd_step', ptr(p), ptr(g), ptr(mom), ptr(ema_in), ptr(ema_out), ptr(g2), ptr(offsets), n_seg, n, ptr(items), items.shape[0], ptr(seg_first), ptr(item_part), float(max_norm or 0.0), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(dampening)), int(first), ptr(loss_gate), ptr(total_norm), float(grad_scale), ptr(p16), _lib.BF16 if p16 is None else dtype_code(p16.dtype), ptr(s_in), ptr(s_out), ptr(lr_dev), stream_ptr())


# ------------------------------------------------------------------------------------------------ forced alignment

def ctc_alignment(log_probs_btc, targets, input_lengths, target_lengths, blank):
	"""log_probs_btc: contiguous (B, T, C) fp32 on the GPU.  Returns (B, S_max) int64 (see include/convasr_hip.h)."""
	B, T, C = log_probs_btc.shape
	dev = log_probs_btc.device
	assert log_probs_btc.is_contiguous() and log_probs_btc.dtype == torch.float32
	targets, il, tl = _ctc_targets(targets, input_lengths, target_lengths, B, dev)
	S_max = targets.shape[1]
	out = torch.empty(B, S_max, dtype = torch.int64, device = dev)
	ws = workspace(_lib.load().convasr_ctc_alignment_workspace_bytes(B, T, S_max), dev, 'ctc_alignment')  # (asked every time, not _cached_query: the answer follows the library's debug bits -- which of the two kernels runs -- as well as the arguments)
	call('convasr_ctc_alignment', ptr(log_probs_btc), ptr(targets), ptr(il), ptr(tl), ptr(out), ptr(ws), B, T, C, S_max, int(blank), stream_ptr())
	return out


ALIGN_LONG_WORKSPACE_CAP = 16 << 30  # bytes of workspace one convasr_ctc_alignment_long call may take; a resource bound like NW_WORKSPACE_CAP, not a measurement


def ctc_alignment_long_tiles():
	"""(states per block, default frames per chunk) of convasr_ctc_alignment_long's tiles (tests straddle them)."""
	return _cached_query('convasr_ctc_alignment_long_states_per_block'), _cached_query('convasr_ctc_alignment_long_chunk_frames')


def ctc_alignment_long(log_probs_btc, targets, input_lengths, target_lengths, blank, chunk_frames = 0, workspace_cap = ALIGN_LONG_WORKSPACE_CAP):
	"""ctc_alignment for whole recordings (include/convasr_hip.h: convasr_ctc_alignment_long): up to 131,071 labels and 2^20 frames, the same
	result as ctc_alignment where that takes the targets.  chunk_frames: 0 = the default tile length, 16 .. 4096 forces it.  The workspace
	(about 4.9 GB for an hour) is allocated for this call and goes back to the allocator; a need above workspace_cap raises ConvasrHipError."""
	B, T, C = log_probs_btc.shape
	dev = log_probs_btc.device
	require_cuda(log_probs_btc)
	assert log_probs_btc.is_contiguous() and log_probs_btc.dtype == torch.float32
	targets, il, tl = _ctc_targets(targets, input_lengths, target_lengths, B, dev)
	S_max = targets.shape[1]
	nbytes = _query('convasr_ctc_alignment_long_workspace_bytes', B, T, S_max)
	ws = _call_workspace(nbytes, dev, workspace_cap, 'ctc_alignment_long', f'B {B}, T {T}, S_max {S_max}')
	out = torch.empty(B, S_max, dtype = torch.int64, device = dev)
	call('convasr_ctc_alignment_long', ptr(log_probs_btc), ptr(targets), ptr(il), ptr(tl), ptr(out), ptr(ws), nbytes, B, T, C, S_max, int(blank), int(chunk_frames), stream_ptr())
	return out


STAR_ALIGN_WORKSPACE_CAP = 16 << 30  # bytes of workspace one convasr_star_alignment call may take; a resource bound like ALIGN_LONG_WORKSPACE_CAP, not a measurement
STAR_ALIGN_MAX_LABELS, STAR_ALIGN_MAX_FRAMES, STAR_ALIGN_MAX_BATCH = 131071, 1 << 20, 65535  # the envelope of convasr_star_alignment (the library checks it again)


def star_alignment_tiles():
	"""(states per block, default frames per chunk) of convasr_star_alignment's tiles (tests straddle them)."""
	return _cached_query('convasr_star_alignment_states_per_block'), _cached_query('convasr_star_alignment_chunk_frames')


def star_alignment_units(targets, target_lengths, star_mask, C):
	"""The unit table convasr_star_alignment reads, built on the targets' device by cumsum and scatter: targets (B, S_max) int64,
	target_lengths (B,), star_mask (B, S_max + 1) bool -> (units (B, 2 S_max + 1) int32, n_units (B,) int32).  Row b lists a star,
	-(gap + 2), ahead of label g for every allowed gap g <= target_lengths[b], and every label's class (-1 where it lies outside [0, C))."""
	B, S_max = targets.shape
	g = torch.arange(S_max + 1, device = targets.device).unsqueeze(0)
	ylen = target_lengths.clamp(0, S_max).unsqueeze(1)
	m = (star_mask & (g <= ylen)).to(torch.int64)
	at = g + m.cumsum(dim = 1) - m  # the unit index of gap g's star; its label follows at + m
	N = 2 * S_max + 1
	units = torch.zeros(B, N + 1, dtype = torch.int32, device = targets.device)  # (column N takes what has no unit)
	units.scatter_(1, torch.where(m > 0, at, N), (-(g + 2)).to(torch.int32).expand(B, -1))
	cls = torch.where((targets >= 0) & (targets < C), targets, -1).to(torch.int32)
	units.scatter_(1, torch.where(g[:, :S_max] < ylen, (at + m)[:, :S_max], N), cls)
	return units[:, :N], (ylen.squeeze(1) + m.sum(dim = 1)).to(torch.int32)


def star_ctc_alignment(log_probs_btc, targets, input_lengths, target_lengths, blank, star_mask, star_penalty, star_enter, chunk_frames = 0, workspace_cap = STAR_ALIGN_WORKSPACE_CAP, parts = 3, _reuse = None):
	"""The best path of a partial transcript through a whole recording (include/convasr_hip.h: convasr_star_alignment has the rule): the
	star lattice of star_ctc_loss, max-plus Viterbi in fp32, up to 131,071 labels and 2^20 frames.  log_probs_btc contiguous (B, T, C) fp32,
	star_mask (B, S_max + 1) bool, star_penalty / star_enter finite natural-log costs <= 0 (no defaults: nothing is tuned).  Returns a
	namespace: alignment (B, S_max) int64 -- the last frame inside every label's state, ctc_alignment's convention --, star_begin and
	star_frames (B, S_max + 1) int64 -- the first frame and the number of frames gap g's star absorbed, -1 and 0 where it is unused --,
	score (B,) fp32, -inf where no path exists -- and input_lengths as the kernel read them (ctc.star_pieces wants them).  chunk_frames: 0 = the default tile length, 16 .. 4096 forces it (no output depends on
	it).  The workspace is allocated for this call; a need above workspace_cap raises ConvasrHipError.  Eager only: the widest row's unit
	count is read back to size the lattice.  parts / _reuse: measurements time the sweep (1) and the walk (2) apart over one workspace."""
	if log_probs_btc.ndim != 3:
		raise ValueError(f'star_ctc_alignment: log_probs (B, T, C) expected, got {tuple(log_probs_btc.shape)}')
	B, T, C = log_probs_btc.shape
	for name, v in (('star_penalty', star_penalty), ('star_enter', star_enter)):
		if not isinstance(v, (int, float)) or isinstance(v, bool) or not v <= 0 or v == float('-inf'):
			raise ValueError(f'star_ctc_alignment: {name} must be a finite natural-log cost <= 0, got {v!r}')
	chunk_frames = int(chunk_frames)
	if chunk_frames != 0 and not 16 <= chunk_frames <= 4096:
		raise ValueError(f'star_ctc_alignment: chunk_frames {chunk_frames} is neither 0 nor in [16, 4096]')
	if not 0 <= int(blank) < C:
		raise ValueError(f'star_ctc_alignment: blank {blank} is outside [0, {C})')
	targets = targets.view(B, -1) if targets.ndim == 1 else targets
	S_max = targets.shape[1]
	if targets.shape[0] != B or tuple(input_lengths.shape) != (B,) or tuple(target_lengths.shape) != (B,):
		raise ValueError(f'star_ctc_alignment: targets (B, S_max) and lengths (B,) expected for a batch of {B}, got {tuple(targets.shape)}, {tuple(input_lengths.shape)}, {tuple(target_lengths.shape)}')
	if tuple(star_mask.shape) != (B, S_max + 1) or star_mask.dtype != torch.bool:
		raise ValueError(f'star_ctc_alignment: a bool star_mask of shape {(B, S_max + 1)} expected, got {star_mask.dtype} {tuple(star_mask.shape)}')
	if B < 1 or T < 1 or B > STAR_ALIGN_MAX_BATCH or T > STAR_ALIGN_MAX_FRAMES or S_max > STAR_ALIGN_MAX_LABELS:
		raise _lib.ConvasrHipError(f'star_ctc_alignment: B {B}, T {T}, S_max {S_max} outside the envelope (1 <= B <= {STAR_ALIGN_MAX_BATCH}, 1 <= T <= {STAR_ALIGN_MAX_FRAMES}, S_max <= {STAR_ALIGN_MAX_LABELS})')
	require_cuda(log_probs_btc)
	dev = log_probs_btc.device
	assert log_probs_btc.is_contiguous() and log_probs_btc.dtype == torch.float32
	targets, il, tl = _ctc_targets(targets, input_lengths, target_lengths, B, dev)
	if _reuse is None:
		units, n_units = star_alignment_units(targets, tl, star_mask.to(dev), C)
		N_max = max(1, int(n_units.max()))  # (a read-back: the lattice and its workspace are as wide as the widest row, not as 2 S_max + 1)
		units = units[:, :N_max].contiguous()
		nbytes = _query('convasr_star_alignment_workspace_bytes', B, T, N_max)
		ws = _call_workspace(nbytes, dev, workspace_cap, 'star_ctc_alignment', f'B {B}, T {T}, {N_max} units')
	else:
		units, n_units, N_max, nbytes, ws = _reuse
	out = types.SimpleNamespace(alignment = torch.empty(B, S_max, dtype = torch.int64, device = dev), star_begin = torch.empty(B, S_max + 1, dtype = torch.int64, device = dev),
	                            star_frames = torch.empty(B, S_max + 1, dtype = torch.int64, device = dev), score = torch.empty(B, dtype = torch.float32, device = dev), input_lengths = il)
	call('convasr_star_alignment_parts', ptr(log_probs_btc), ptr(units), ptr(n_units), ptr(il), ptr(tl), float(star_penalty), float(star_enter), ptr(out.alignment), ptr(out.star_begin),
	     ptr(out.star_frames), ptr(out.score), ptr(ws), nbytes, B, T, C, S_max, N_max, int(blank), chunk_frames, int(parts), stream_ptr())
	if parts != 3:
		out._reuse = (units, n_units, N_max, nbytes, ws)
	return out


# ------------------------------------------------------------------------------------------------ keyword search

def ctc_keyword_search_limits():
	"""(labels per phrase at most, phrases per workgroup, classes up to which frames are staged through LDS) of convasr_ctc_keyword_search
	(tests straddle them)."""
	return _cached_query('convasr_ctc_keyword_search_max_labels'), _cached_query('convasr_ctc_keyword_search_phrases_per_block'), _cached_query('convasr_ctc_keyword_search_staged_classes')


def ctc_keyword_search_tile_frames(C):
	"""Frames of one tile of convasr_ctc_keyword_search at C classes (tests straddle it)."""
	return _query('convasr_ctc_keyword_search_tile_frames', int(C))


def ctc_keyword_search(log_probs, tokens, token_lengths, blank, thresholds, lengths = None, min_gap = 10, max_hits = 16, dense = False):
	"""Where in every utterance each of K phrases is said (include/convasr_hip.h: convasr_ctc_keyword_search has the rule).  log_probs (B, C, T)
	log-probs or logits; tokens (K, L_max) and token_lengths (K,) integers (a tensor, an array or lists); thresholds a float or (K,) values;
	lengths (B,) frames or None; min_gap in frames.  Returns a namespace of device tensors: count (B, K) int32, score fp32 / begin / end int32
	(B, K, H) with the first count[b, k] entries of a row filled (the rest -inf / -1) and dense_score / dense_begin (B, K, T) or None.  H is
	max_hits, or the largest count where that is more: the search then runs once more at that capacity, so no hit is dropped (the count is
	read on the host: one synchronisation).  A label equal to blank or outside [0, C), an empty phrase or phrase list and shapes that do not
	fit raise ValueError before any launch; outside the kernel's envelope (a phrase of more than 64 labels, ...) ConvasrHipError."""
	require_cuda(log_probs)
	if log_probs.ndim != 3:
		raise ValueError(f'ctc_keyword_search: (B, C, T) log-probs expected, got shape {tuple(log_probs.shape)}')
	B, C, T = log_probs.shape
	tok, tl = torch.as_tensor(tokens).cpu(), torch.as_tensor(token_lengths).cpu()
	if tok.ndim != 2 or tok.shape[0] < 1 or tok.shape[1] < 1 or tok.dtype.is_floating_point:
		raise ValueError(f'ctc_keyword_search: tokens must be (K, L_max) integers with K, L_max >= 1, got shape {tuple(tok.shape)}')
	K = tok.shape[0]
	if tl.shape != (K,) or tl.dtype.is_floating_point or int(tl.min()) < 1 or int(tl.max()) > tok.shape[1]:
		raise ValueError(f'ctc_keyword_search: token_lengths must be (K,) = ({K},) integers in [1, {tok.shape[1]}], got shape {tuple(tl.shape)}')
	if not -C <= int(blank) < C:
		raise ValueError(f'ctc_keyword_search: blank {blank} for {C} classes')
	blank = int(blank) % C
	if int(min_gap) < 0 or int(max_hits) < 1:
		raise ValueError(f'ctc_keyword_search: min_gap {min_gap} must be >= 0 and max_hits {max_hits} >= 1')
	tok = tok[:, :int(tl.max())].to(torch.int64)
	used = torch.arange(tok.shape[1]).unsqueeze(0) < tl.unsqueeze(1)
	if bool(((tok == blank) & used).any()):
		raise ValueError(f'ctc_keyword_search: a phrase holds the blank {blank}')
	if bool((((tok < 0) | (tok >= C)) & used).any()):
		raise ValueError(f'ctc_keyword_search: a label outside [0, {C})')
	dev = log_probs.device
	thr = torch.as_tensor(thresholds, dtype = torch.float32)
	thr = thr.expand(K) if thr.ndim == 0 else thr
	if thr.shape != (K,):
		raise ValueError(f'ctc_keyword_search: thresholds of shape {tuple(thr.shape)} for {K} phrases')
	thr = thr.to(dev).contiguous()
	lengths = None if lengths is None else _frame_lengths('ctc_keyword_search', lengths, B, T, dev)
	lp = as_cl(log_probs, torch.float32)
	tok, tl = (tok * used).to(device = dev, dtype = torch.int32).contiguous(), tl.to(device = dev, dtype = torch.int32).contiguous()
	count = torch.empty(B, K, dtype = torch.int32, device = dev)
	dense_score = torch.empty(B, K, T, dtype = torch.float32, device = dev) if dense else None
	dense_begin = torch.empty(B, K, T, dtype = torch.int32, device = dev) if dense else None
	H = int(max_hits)
	while True:
		score = torch.full((B, K, H), float('-inf'), dtype = torch.float32, device = dev)
		begin, end = torch.full((2, B, K, H), -1, dtype = torch.int32, device = dev).unbind(0)
		call('convasr_ctc_keyword_search', ptr(lp), ptr(lengths), ptr(tok), ptr(tl), ptr(thr), ptr(count), ptr(score), ptr(begin), ptr(end), ptr(dense_score), ptr(dense_begin),
		     B, T, C, K, tok.shape[1], H, blank, int(min_gap), stream_ptr())
		most = int(count.max())
		if most <= H:
			return types.SimpleNamespace(count = count, score = score, begin = begin, end = end, dense_score = dense_score, dense_begin = dense_begin)
		H = most


# ------------------------------------------------------------------------------------------------ decoding

def _beam_route(name, args, wide):
	"""(entry point, workspace bytes): the LDS kernel whenever its workspace query accepts the arguments (wide None), otherwise -- or with
	wide True -- the wide one (beam state in the workspace, beam_width <= 8192); wide False keeps the LDS kernel.  Raises ConvasrHipError
	with the refusing query's message."""
	lib = _lib.load()
	if not wide:
		nbytes = getattr(lib, f'convasr_{name}_workspace_bytes')(*args)
		if nbytes >= 0 or wide is False:
			if nbytes < 0:
				raise _lib.ConvasrHipError(lib.convasr_last_error().decode())
			return f'convasr_{name}', nbytes
	nbytes = getattr(lib, f'convasr_{name}_wide_workspace_bytes')(*args)
	if nbytes < 0:
		raise _lib.ConvasrHipError(lib.convasr_last_error().decode())
	return f'convasr_{name}_wide', nbytes


def ctc_beam_search(log_probs_bct, lengths, blank, beam_width, cutoff_top_n = 40, cutoff_prob = 1.0, topk = 1, *, wide = None):
	"""CTC prefix beam search without a language model (include/convasr_hip.h: convasr_ctc_beam_search).  log_probs_bct: (B, C, T) log-probs
	on the GPU (the model's channels-last fp32 is read in place, anything else is converted); lengths (B,) frames per utterance or None (all T).
	Returns (tokens (B, topk, T) int64, offsets (B, topk, T) int32, out_lengths (B, topk) int64, log_prob (B, topk) fp32), best first.
	cutoff_top_n above C means C.  beam_width <= 1024 (and the LDS budget) runs the LDS kernel; wider beams, up to 8192, run the wide one
	(convasr_ctc_beam_search_wide: the same search, the beam state in the workspace).  wide: None chooses so, True forces the wide kernel,
	False the LDS one.  The workspace is allocated for the call: B x T x beam_width x 8 bytes of prefix-node arena, plus the wide kernel's
	beam state (1.9 GB in all at 64 x 750 x 5000).  Outside the envelope (beam_width <= 8192, cutoff_top_n <= 128, C <= 8192, ...) it
	raises ConvasrHipError."""
	require_cuda(log_probs_bct)
	B, C, T = log_probs_bct.shape
	lp = as_cl(log_probs_bct, torch.float32)
	dev = lp.device
	lengths = _frame_lengths('ctc_beam_search', lengths, B, T, dev)
	N = C if cutoff_top_n is None else min(int(cutoff_top_n), C)  # (ctcdecode's pruning takes min(cutoff_top_n, C) too: the reference's default 40 over its 38 classes)
	W, topk = int(beam_width), int(topk)
	fn, nbytes = _beam_route('ctc_beam_search', (B, T, C, W, N, topk), wide)
	tokens = torch.empty(B, topk, T, dtype = torch.int64, device = dev)
	offsets = torch.empty(B, topk, T, dtype = torch.int32, device = dev)
	out_lengths = torch.empty(B, topk, dtype = torch.int64, device = dev)
	log_prob = torch.empty(B, topk, dtype = torch.float32, device = dev)
	ws = _call_workspace(nbytes, dev)  # B x T x W nodes of 8 bytes: 393 MB at 64 x 750 x 1024
	call(fn, ptr(lp), ptr(lengths), ptr(tokens), ptr(offsets), ptr(out_lengths), ptr(log_prob), ptr(ws), B, T, C, int(blank), W, N, float(cutoff_prob), topk, stream_ptr())
	return tokens, offsets, out_lengths, log_prob


def ctc_beam_search_lm(log_probs_bct, lengths, blank, beam_width, lm, alpha, beta, cutoff_top_n = 40, cutoff_prob = 1.0, topk = 1, *, wide = None):
	"""CTC prefix beam search fused with an n-gram LM (include/convasr_hip.h: convasr_ctc_beam_search_lm).  lm: an lm.NgramLM built for
	the C labels of log_probs_bct (its tables are uploaded to the device once and kept by the model); alpha / beta weigh the LM term.
	Inputs, outputs and `wide` as ctc_beam_search, except log_prob: (B, topk) fp64, the fused score lpb + lpnb + F (best first).  A width
	the LDS kernel's budget refuses runs the wide kernel (convasr_ctc_beam_search_lm_wide).  Outside the envelope (that of ctc_beam_search
	plus C <= 256, see the header) it raises ConvasrHipError."""
	require_cuda(log_probs_bct)
	B, C, T = log_probs_bct.shape
	if C != lm.num_classes:
		raise ValueError(f'ctc_beam_search_lm: {C} classes, but the language model was built for {lm.num_classes} labels')
	if lm.space == int(blank):
		raise ValueError(f'ctc_beam_search_lm: the space class {lm.space} is the blank')
	lp = as_cl(log_probs_bct, torch.float32)
	dev = lp.device
	lengths = _frame_lengths('ctc_beam_search_lm', lengths, B, T, dev)
	N = C if cutoff_top_n is None else min(int(cutoff_top_n), C)
	W, topk = int(beam_width), int(topk)
	fn, nbytes = _beam_route('ctc_beam_search_lm', (B, T, C, W, N, topk), wide)
	t = lm.device_tables(int(blank), dev)
	tokens = torch.empty(B, topk, T, dtype = torch.int64, device = dev)
	offsets = torch.empty(B, topk, T, dtype = torch.int32, device = dev)
	out_lengths = torch.empty(B, topk, dtype = torch.int64, device = dev)
	log_prob = torch.empty(B, topk, dtype = torch.float64, device = dev)
	ws = _call_workspace(nbytes, dev)
	call(fn, ptr(lp), ptr(lengths), ptr(tokens), ptr(offsets), ptr(out_lengths), ptr(log_prob), ptr(ws), B, T, C, int(blank), W, N,
	     float(cutoff_prob), topk, ptr(t['node_mask']), ptr(t['node_child']), ptr(t['node_word']), int(t['node_word'].numel()), ptr(t['ent_pb']), ptr(t['ent_sl']),
	     int(t['ent_sl'].shape[0]), ptr(t['slots']), int(t['slots'].shape[0]), lm.space, lm.order, lm.start_state, float(alpha), float(beta), stream_ptr())
	return tokens, offsets, out_lengths, log_prob


def ctc_beam_search_hot(log_probs_bct, lengths, blank, beam_width, hot, weight, lm = None, alpha = 0.0, beta = 0.0, cutoff_top_n = 40, cutoff_prob = 1.0, topk = 1, *,
                        wide = None):
	"""CTC prefix beam search biased towards a list of hot phrases (include/convasr_hip.h: convasr_ctc_beam_search_hot).  hot: a
	hotwords.HotWords built for the C labels of log_probs_bct (its tables are uploaded to the device once and kept by it); weight >= 0,
	in natural-log units per matched label: a hypothesis gains weight for every label of a listed phrase it spells in full, starting at
	the beginning of the utterance or after a space, and nothing for a phrase it leaves unfinished.  No weight has been tuned on speech
	here, so there is no default.  lm: None, or an lm.NgramLM for the same labels, fused as ctc_beam_search_lm does with alpha / beta
	(convasr_ctc_beam_search_lm_hot); every word of every phrase must then be in its vocabulary (ValueError otherwise).
	Inputs, outputs and `wide` as ctc_beam_search, except log_prob: (B, topk) fp64 with or without an LM, the ranking score lpb + lpnb
	(+ the LM's F) + F_hot, best first.  C <= 256.  Without an LM the LDS kernel takes beam_width 1024 at every C <= 256; with an LM at
	C <= 96 and cutoff_top_n <= 64 (C = 38 among them), and e.g. 814 at C = 256 (the header lists the widths); a width its budget refuses
	runs the wide kernel (beam_width <= 8192), with the same results.  weight = 0
	or an empty list is the search of ctc_beam_search / ctc_beam_search_lm.  Outside the envelope it raises ConvasrHipError."""
	require_cuda(log_probs_bct)
	B, C, T = log_probs_bct.shape
	blank, weight = int(blank), float(weight)
	if C != hot.num_classes:
		raise ValueError(f'ctc_beam_search_hot: {C} classes, but the hot phrases were built for {hot.num_classes} labels')
	if not (math.isfinite(weight) and weight >= 0.0):
		raise ValueError(f'ctc_beam_search_hot: the weight {weight} must be finite and >= 0')
	name = 'ctc_beam_search_hot'
	if lm is not None:
		name = 'ctc_beam_search_lm_hot'
		if C != lm.num_classes or lm.space != hot.space:
			raise ValueError(f'ctc_beam_search_hot: the language model was built for other labels ({lm.num_classes} classes, space {lm.space}) than the hot phrases ({C}, {hot.space})')
		hot.check_vocabulary(lm, blank)
	lp = as_cl(log_probs_bct, torch.float32)
	dev = lp.device
	h = hot.device_tables(blank, dev)  # (ValueError for a phrase with the blank's character, or a blank that is the space)
	lengths = _frame_lengths(name, lengths, B, T, dev)
	N = C if cutoff_top_n is None else min(int(cutoff_top_n), C)
	W, topk = int(beam_width), int(topk)
	fn, nbytes = _beam_route(name, (B, T, C, W, N, topk), wide)
	tokens = torch.empty(B, topk, T, dtype = torch.int64, device = dev)
	offsets = torch.empty(B, topk, T, dtype = torch.int32, device = dev)
	out_lengths = torch.empty(B, topk, dtype = torch.int64, device = dev)
	log_prob = torch.empty(B, topk, dtype = torch.float64, device = dev)
	ws = _call_workspace(nbytes, dev)
	hot_args = (ptr(h['hot_mask']), ptr(h['hot_child']), ptr(h['hot_term']), int(h['hot_term'].numel()), int(h['hot_mask'].shape[1]))
	head = (ptr(lp), ptr(lengths), ptr(tokens), ptr(offsets), ptr(out_lengths), ptr(log_prob), ptr(ws), B, T, C, blank, W, N, float(cutoff_prob), topk)
	if lm is None:
		call(fn, *head, *hot_args, hot.space, weight, stream_ptr())
	else:
		t = lm.device_tables(blank, dev)
		call(fn, *head, ptr(t['node_mask']), ptr(t['node_child']), ptr(t['node_word']), int(t['node_word'].numel()), ptr(t['ent_pb']), ptr(t['ent_sl']),
		     int(t['ent_sl'].shape[0]), ptr(t['slots']), int(t['slots'].shape[0]), lm.space, lm.order, lm.start_state, float(alpha), float(beta), *hot_args, weight, stream_ptr())
	return tokens, offsets, out_lengths, log_prob


def ctc_greedy_collapse(path, lengths, eps, space, blank_amount_to_space = 10):
	"""GreedyCTCGenerator.generate's collapse (time_stamps None, silence = {eps, space}, word start = space) on the device
	(include/convasr_hip.h: convasr_ctc_greedy_collapse).  path: (B, T) int64 per-frame argmax (ops.argmax); lengths (B,) frames, or None
	(all T).  Returns (tokens (B, T) int64, 0 past the length; out_lengths (B,) int64).  Outside the envelope it raises ConvasrHipError."""
	require_cuda(path)
	if path.ndim != 2 or path.dtype != torch.int64:
		raise ValueError(f'ctc_greedy_collapse: path must be a (B, T) int64 tensor, got {tuple(path.shape)} {path.dtype}')
	B, T = path.shape
	dev = path.device
	path = path.contiguous()
	lengths = _frame_lengths('ctc_greedy_collapse', lengths, B, T, dev)
	tokens = torch.empty(B, T, dtype = torch.int64, device = dev)
	out_lengths = torch.empty(B, dtype = torch.int64, device = dev)
	call('convasr_ctc_greedy_collapse', ptr(path), ptr(lengths), ptr(tokens), ptr(out_lengths), B, T, int(eps), int(space), int(blank_amount_to_space), stream_ptr())
	return tokens, out_lengths


def ctc_greedy_segments_chunk():
	"""Frames per chunk of convasr_ctc_greedy_segments (one workgroup per utterance and chunk; tests straddle it)."""
	return _cached_query('convasr_ctc_greedy_segments_chunk_frames')


def ctc_greedy_segments(path, lengths, eps, space, blank_amount_to_space = 10, split_words = True):
	"""GreedyCTCGenerator.generate's collapse with the frame of every token and the word segments, on the device (include/convasr_hip.h:
	convasr_ctc_greedy_segments has the rule).  path: (B, T) int64 per-frame argmax (ops.argmax); lengths (B,) frames, or None (all T).
	split_words: every space emitted from the path opens a segment and stands twice at its front (time stamps given); False: one segment
	per non-empty utterance.  Returns device tensors, packed over the batch in utterance order: tokens (n,) int64, frames (n,) int32,
	counts (2, B) int64 (tokens, then segments, per utterance), seg_first (m,) int64 (index of a segment's first token in tokens),
	seg_begin / seg_end (m,) int32 frames.  One read-back, of the counts (16 B bytes), sizes the results.  Outside the envelope it raises
	ConvasrHipError."""
	require_cuda(path)
	if path.ndim != 2 or path.dtype != torch.int64:
		raise ValueError(f'ctc_greedy_segments: path must be a (B, T) int64 tensor, got {tuple(path.shape)} {path.dtype}')
	B, T = path.shape
	dev = path.device
	path = path.contiguous()
	lengths = _frame_lengths('ctc_greedy_segments', lengths, B, T, dev)
	nbytes = _query('convasr_ctc_greedy_segments_workspace_bytes', B, T)
	room = B * T * (2 if split_words else 1)
	tokens = torch.empty(room, dtype = torch.int64, device = dev)
	frames = torch.empty(room, dtype = torch.int32, device = dev)
	counts = torch.empty(2, B, dtype = torch.int64, device = dev)
	seg_first = torch.empty(B * T, dtype = torch.int64, device = dev)
	seg_begin = torch.empty(B * T, dtype = torch.int32, device = dev)
	seg_end = torch.empty(B * T, dtype = torch.int32, device = dev)
	ws = _call_workspace(nbytes, dev)
	call('convasr_ctc_greedy_segments', ptr(path), ptr(lengths), ptr(tokens), ptr(frames), ptr(counts), ptr(seg_first), ptr(seg_begin), ptr(seg_end),
	     ptr(ws), nbytes, B, T, int(eps), int(space), int(blank_amount_to_space), int(bool(split_words)), stream_ptr())
	n, m = counts.sum(dim = 1).tolist()
	return tokens[:n], frames[:n], counts, seg_first[:m], seg_begin[:m], seg_end[:m]


# ------------------------------------------------------------------------------------------------ metrics and alignment

def edit_distance(hyp, hyp_lengths, ref, ref_lengths, mode = _lib.METRIC_CHARS, space = -1):
	"""Levenshtein distances of hypotheses against references (include/convasr_hip.h: convasr_edit_distance).  hyp: (B, K, Lh) or (B, Lh)
	int64 tokens with hyp_lengths (B, K) / (B,); ref: (B, Lr) int64, rows read in place through their stride (y[:, 0] of a (B, n, Lpad)
	batch needs no copy), ref_lengths (B,) read through its stride as well (ylen[:, 0]).  mode: _lib.METRIC_CHARS (units = the tokens that
	are not `space`; space < 0: every token) or _lib.METRIC_WORDS (units = maximal runs of non-space tokens, space >= 0).
	Returns (distance (B, K) int32 -- (B,) for a (B, Lh) hyp -- , ref_units (B,) int32).  Outside the envelope (Lh, Lr <= 16383,
	B * K < 2^20, ...) it raises ConvasrHipError; edit_distance_long takes longer pairs (of ready-made unit ids)."""
	require_cuda(hyp, ref)
	squeeze = hyp.ndim == 2
	if squeeze:
		hyp, hyp_lengths = hyp.unsqueeze(1), torch.as_tensor(hyp_lengths).unsqueeze(1)
	if hyp.ndim != 3 or ref.ndim != 2 or hyp.shape[0] != ref.shape[0]:
		raise ValueError(f'edit_distance: hyp {tuple(hyp.shape)} and ref {tuple(ref.shape)} are not (B, K, Lh) and (B, Lr)')
	B, K, Lh = hyp.shape
	Lr = ref.shape[1]
	dev = hyp.device
	if hyp.dtype != torch.int64 or ref.dtype != torch.int64:
		raise ValueError('edit_distance: hyp and ref must be int64 tokens')
	hyp = hyp.contiguous()
	if Lh == 0:  # (a zero-size tensor has no storage to point at; no token is read past a length anyway)
		hyp = torch.zeros(B, K, 1, dtype = torch.int64, device = dev)
	if Lr == 0 or ref.stride(1) != 1:
		ref = torch.zeros(B, 1, dtype = torch.int64, device = dev) if Lr == 0 else ref.contiguous()
	hyp_lengths = torch.as_tensor(hyp_lengths).to(device = dev, dtype = torch.int64).reshape(B, K).contiguous()
	ref_lengths = torch.as_tensor(ref_lengths).to(device = dev, dtype = torch.int64)
	if ref_lengths.shape != (B,):
		raise ValueError(f'edit_distance: ref_lengths of shape {tuple(ref_lengths.shape)} for a batch of {B}')
	distance = torch.empty(B, K, dtype = torch.int32, device = dev)
	ref_units = torch.empty(B, dtype = torch.int32, device = dev)
	call('convasr_edit_distance', ptr(hyp), ptr(hyp_lengths), ptr(ref), ref.stride(0), ptr(ref_lengths), ref_lengths.stride(0), ptr(distance), ptr(ref_units),
	     B, K, Lh, Lr, int(mode), int(space), stream_ptr())
	return (distance[:, 0] if squeeze else distance), ref_units


NW_WORKSPACE_CAP = 1 << 30  # bytes of direction workspace one convasr_nw_align launch may take; a resource bound, not a measurement


def nw_align_workspace_bytes(N, La, Lb):
	"""convasr_nw_align_workspace_bytes: N * La * ceil(Lb / 64) * 16 + N * (La + Lb) * 4."""
	return _query('convasr_nw_align_workspace_bytes', int(N), int(La), int(Lb))


NW_LONG_WORKSPACE_CAP = 16 << 30  # bytes of workspace one convasr_nw_align_long / convasr_edit_distance_long call may take; a resource bound like ALIGN_LONG_WORKSPACE_CAP, not a measurement
NW_LONG_MAX_LEN = 131071  # CONVASR_NW_LONG_MAX_LEN


def nw_align_long_tile():
	"""The edge of convasr_nw_align_long's (and convasr_edit_distance_long's) square tiles, in cells (tests straddle it)."""
	return _cached_query('convasr_nw_align_long_tile')


def nw_align_long_workspace_bytes(N, La, Lb):
	"""convasr_nw_align_long_workspace_bytes (include/convasr_hip.h states the formula)."""
	return _query('convasr_nw_align_long_workspace_bytes', int(N), int(La), int(Lb))


def edit_distance_long_workspace_bytes(N, La, Lb):
	"""convasr_edit_distance_long_workspace_bytes: the two boundary families of include/convasr_hip.h."""
	return _query('convasr_edit_distance_long_workspace_bytes', int(N), int(La), int(Lb))


def _pairs(name, a, a_lengths, b, b_lengths):
	"""N pairs of unit ids as the alignment kernels read them: a (N, La) and b (N, Lb) int32, contiguous, with (N,) int32 lengths, all on a's device."""
	require_cuda(a, b)
	if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
		raise ValueError(f'{name}: a {tuple(a.shape)} and b {tuple(b.shape)} are not (N, La) and (N, Lb)')
	dev = a.device
	N = a.shape[0]
	a, b = a.to(torch.int32).contiguous(), b.to(device = dev, dtype = torch.int32).contiguous()
	al = torch.as_tensor(a_lengths).to(device = dev, dtype = torch.int32).contiguous()
	bl = torch.as_tensor(b_lengths).to(device = dev, dtype = torch.int32).contiguous()
	if al.shape != (N,) or bl.shape != (N,):
		raise ValueError(f'{name}: lengths of shapes {tuple(al.shape)}, {tuple(bl.shape)} for a batch of {N}')
	return a, al, b, bl


def _units(x):
	"""x, or a one-column stand-in for an (N, 0) tensor: a zero-size tensor has no storage to point at (no unit is read past a length anyway)."""
	return x if x.shape[1] else torch.zeros(x.shape[0], 1, dtype = torch.int32, device = x.device)


def _cap_groups(la, lb, need, cap):
	"""The split ops.nw_align makes of a batch over its workspace cap: the pairs p (of la[p] x lb[p] units) ordered by need(1, la[p], lb[p]),
	largest first, and cut into the fewest groups that each fit under `cap` at their own largest lengths.  Returns [(members, group La,
	group Lb)]; the first group holds the largest pair (which alone may still be over the cap: the caller checks)."""
	order = sorted(range(len(la)), key = lambda p: -need(1, la[p], lb[p]))
	groups, cur, ga, gb = [], [], 0, 0
	for p in order:
		na, nb = max(ga, la[p]), max(gb, lb[p])
		if cur and need(len(cur) + 1, na, nb) > cap:
			groups.append((cur, ga, gb))
			cur, na, nb = [], la[p], lb[p]
		cur, ga, gb = cur + [p], na, nb
	groups.append((cur, ga, gb))
	return groups


def _launch_pairs(name, query, launch, a, al, b, bl, workspace_cap):
	"""launch(a, al, b, bl) -> tuple of per-pair results, over the whole batch while query(N, La, Lb) bytes of workspace fit under the cap
	(nothing is copied to the host).  A larger batch is split: the lengths come to the host once, _cap_groups cuts it, and every group is
	launched at its own largest lengths and scattered back -- (N,) results whole, index rows into the first columns of (N, La + Lb) rows of -1."""
	N, La, Lb = a.shape[0], a.shape[1], b.shape[1]
	if query(N, La, Lb) <= workspace_cap:
		return launch(a, al, b, bl)
	lens = torch.stack([al.clamp(0, La), bl.clamp(0, Lb)]).cpu().tolist()
	groups = _cap_groups(lens[0], lens[1], query, workspace_cap)
	_, ga, gb = groups[0]
	if query(1, ga, gb) > workspace_cap:
		raise _lib.ConvasrHipError(f'{name}: one pair of {ga} x {gb} units needs {query(1, ga, gb)} bytes of workspace, over the cap of {workspace_cap}')
	outs = None
	for members, ga, gb in groups:
		idx = torch.tensor(members, dtype = torch.int64, device = a.device)
		parts = launch(a[idx, :ga].contiguous(), al[idx], b[idx, :gb].contiguous(), bl[idx])
		if outs is None:
			outs = tuple(torch.empty(N, dtype = p.dtype, device = p.device) if p.ndim == 1 else torch.full((N, La + Lb), -1, dtype = p.dtype, device = p.device) for p in parts)
		for out, part in zip(outs, parts):
			if out.ndim == 1:
				out[idx] = part
			else:
				out[idx, :ga + gb] = part
	return outs


def _nw_launch(entry, query, a, al, b, bl, scores, parts = None, ws = None):
	"""One call of convasr_nw_align (parts None) or convasr_nw_align_long_parts (parts 1 = the fill, 2 = the end cell and the walk, 3 = both; ws: a
	workspace of query(N, La, Lb) bytes the caller keeps between the parts)."""
	N, La, Lb = a.shape[0], a.shape[1], b.shape[1]
	dev = a.device
	W = max(La + Lb, 1)
	a_index = torch.empty(N, W, dtype = torch.int32, device = dev)
	b_index = torch.empty(N, W, dtype = torch.int32, device = dev)
	n_cols = torch.empty(N, dtype = torch.int32, device = dev)
	score = torch.empty(N, dtype = torch.int32, device = dev)
	nbytes = query(N, La, Lb)
	ws = _call_workspace(nbytes, dev) if ws is None else ws
	a, b = _units(a), _units(b)
	call(entry, ptr(a), ptr(al), ptr(b), ptr(bl), ptr(a_index), ptr(b_index), ptr(n_cols), ptr(score), ptr(ws), nbytes, N, La, Lb,
	     *scores, *(() if parts is None else (int(parts), )), stream_ptr())
	return a_index[:, :La + Lb], b_index[:, :La + Lb], n_cols, score


def _nw(name, entry, query, parts, a, a_lengths, b, b_lengths, scores, workspace_cap):
	a, al, b, bl = _pairs(name, a, a_lengths, b, b_lengths)
	scores = tuple(int(s) for s in scores)
	if len(scores) != 4:
		raise ValueError(f'{name}: scores = (match, sub, del, ins)')
	return _launch_pairs(name, query, lambda *group: _nw_launch(entry, query, *group, scores, parts), a, al, b, bl, workspace_cap)


def nw_align(a, a_lengths, b, b_lengths, scores, workspace_cap = NW_WORKSPACE_CAP):
	"""Semi-global Needleman-Wunsch alignment with traceback of N pairs (include/convasr_hip.h: convasr_nw_align).  a (N, La) / b (N, Lb):
	integer ids of the hypothesis / reference units (made int32), a_lengths / b_lengths (N,); scores = (match, sub, del, ins), integers in
	[-32768, 32768].  Returns (a_index (N, La + Lb) int32, b_index (N, La + Lb) int32, n_cols (N,) int32, score (N,) int32): per alignment
	column the 0-based unit of a / b or -1 for a gap, -1 past column n_cols; score is the end cell's.

	One launch takes N * La * ceil(Lb / 64) * 16 + N * (La + Lb) * 4 bytes of workspace.  While that is at most workspace_cap (default
	NW_WORKSPACE_CAP = 1 GiB, a resource bound) the whole batch is one launch and nothing is copied to the host.  A larger batch is split:
	the lengths come to the host once, the pairs are ordered by size and cut into the fewest groups that each fit under the cap at their
	own largest lengths, one launch per group.  A single pair over the cap, or anything outside the envelope (N < 2^20, La, Lb <= 16383),
	raises ConvasrHipError; nw_align_long takes longer pairs."""
	return _nw('nw_align', 'convasr_nw_align', nw_align_workspace_bytes, None, a, a_lengths, b, b_lengths, scores, workspace_cap)


def nw_align_long(a, a_lengths, b, b_lengths, scores, workspace_cap = NW_LONG_WORKSPACE_CAP):
	"""nw_align for whole recordings (include/convasr_hip.h: convasr_nw_align_long): up to 131,071 units a side, scores in [-2048, 2048],
	the same four results as nw_align, bit for bit where that takes the arguments.  The matrix is filled in tiles of nw_align_long_tile()
	cells a side, one launch per anti-diagonal of tiles, so one long pair runs on many CUs; not meant for graph capture.

	The workspace (2 direction bits per cell: 16,500 x 16,400 units take 78 MB in all, 100,000 x 100,000 2.5 GB) is allocated for this call and
	goes back to the allocator.  While the batch's need is at most workspace_cap (default NW_LONG_WORKSPACE_CAP = 16 GiB, a resource
	bound) it is one call and nothing is copied to the host; a larger batch is split as nw_align splits one: the lengths come to the host
	once and the pairs are cut into the fewest groups that each fit.  A single pair over the cap, or anything outside the envelope, raises
	ConvasrHipError."""
	return _nw('nw_align_long', 'convasr_nw_align_long_parts', nw_align_long_workspace_bytes, 3, a, a_lengths, b, b_lengths, scores, workspace_cap)


def _ed_long_launch(a, al, b, bl):
	N, La, Lb = a.shape[0], a.shape[1], b.shape[1]
	distance = torch.empty(N, dtype = torch.int32, device = a.device)
	nbytes = edit_distance_long_workspace_bytes(N, La, Lb)
	ws = _call_workspace(nbytes, a.device)
	a, b = _units(a), _units(b)
	call('convasr_edit_distance_long', ptr(a), ptr(al), ptr(b), ptr(bl), ptr(distance), ptr(ws), nbytes, N, La, Lb, stream_ptr())
	return (distance, )


def edit_distance_long(a, a_lengths, b, b_lengths, workspace_cap = NW_LONG_WORKSPACE_CAP):
	"""Levenshtein distances of N pairs of integer unit ids for whole recordings (include/convasr_hip.h: convasr_edit_distance_long): a (N, La)
	/ b (N, Lb) ids (made int32; equal units, equal ids -- the caller makes them, unlike edit_distance), a_lengths / b_lengths (N,), up to
	131,071 units a side.  Returns distance (N,) int32, exact.  The tiles, launches, workspace conventions and the split of a batch over
	workspace_cap are nw_align_long's; the workspace holds the tile boundaries only (4 * (La + Lb) * max(La, Lb) / tile bytes a pair)."""
	a, al, b, bl = _pairs('edit_distance_long', a, a_lengths, b, b_lengths)
	return _launch_pairs('edit_distance_long', edit_distance_long_workspace_bytes, _ed_long_launch, a, al, b, bl, workspace_cap)[0]


# ------------------------------------------------------------------------------------------------ diarization

def sliding_max_tile(kernel_size):
	"""Outputs one workgroup of convasr_sliding_max produces at this window (tests straddle it)."""
	return _query('convasr_sliding_max_tile', int(kernel_size))


def scan_tile():
	"""Elements one workgroup of the prefix sums (sign_prefix_sum, rle1d) scans (tests straddle it)."""
	return _query('convasr_scan_tile')


def sliding_max(x, kernel_size, absolute = False, minimum = False):
	"""F.max_pool1d(x.unsqueeze(1), K, stride = 1, padding = K // 2).squeeze(1) of a (C, L) fp32 device tensor, at a cost that does not depend
	on K (include/convasr_hip.h: convasr_sliding_max).  absolute: of |x|; minimum: the sliding minimum with +inf padding, -max_pool1d(-x).
	Returns (C, L + 2 * (K // 2) - K + 1) fp32.  1 <= K <= 16384, 1 <= L <= 2^28; finite values are assumed, not checked."""
	require_cuda(x)
	if x.ndim != 2 or x.dtype != torch.float32:
		raise ValueError(f'sliding_max: x must be a (C, L) float32 tensor, got {tuple(x.shape)} {x.dtype}')
	C, L = x.shape
	x = x.contiguous()
	out = torch.empty(C, max(_query('convasr_sliding_max_out_len', L, int(kernel_size)), 0), dtype = torch.float32, device = x.device)
	call('convasr_sliding_max', ptr(x), ptr(out), C, L, int(kernel_size), (_lib.SLIDE_ABS if absolute else 0) | (_lib.SLIDE_NEG if minimum else 0), stream_ptr())
	return out


def kth_value(x, k):
	"""x.kthvalue(k, dim = -1).values of a (C, L) fp32 device tensor of NON-NEGATIVE values (not checked), k 1-based: a radix select over the
	bit patterns (convasr_kth_value), exact.  Returns (C,) fp32."""
	require_cuda(x)
	if x.ndim != 2 or x.dtype != torch.float32:
		raise ValueError(f'kth_value: x must be a (C, L) float32 tensor, got {tuple(x.shape)} {x.dtype}')
	C, L = x.shape
	x = x.contiguous()
	nbytes = _query('convasr_kth_value_workspace_bytes', C)
	ws = workspace(nbytes, x.device, 'diar')
	out = torch.empty(C, dtype = torch.float32, device = x.device)
	call('convasr_kth_value', ptr(x), ptr(out), ptr(ws), ws.numel(), C, L, int(k), stream_ptr())
	return out


def sign_prefix_sum(d):
	"""(d[0] - d[1]).sign().cumsum(0) as int32 for a (2, L) fp32 device tensor (convasr_sign_prefix_sum; a multi-workgroup scan)."""
	require_cuda(d)
	if d.ndim != 2 or d.shape[0] != 2 or d.dtype != torch.float32:
		raise ValueError(f'sign_prefix_sum: d must be a (2, L) float32 tensor, got {tuple(d.shape)} {d.dtype}')
	L = d.shape[1]
	d = d.contiguous()
	ws = workspace(_query('convasr_sign_prefix_sum_workspace_bytes', L), d.device, 'diar')
	out = torch.empty(L, dtype = torch.int32, device = d.device)
	call('convasr_sign_prefix_sum', ptr(d), ptr(out), ptr(ws), ws.numel(), L, stream_ptr())
	return out


def select_speaker(signal, kernel_size_smooth_silence, kernel_size_smooth_signal, kernel_size_smooth_speaker, silence_absolute_threshold, silence_relative_threshold, eps, k):
	"""convasr_select_speaker on a (2, N) fp32 device tensor; k = the 1-based rank of the normalisation percentile.  Returns
	(speaker_id (L,) fp32, mask (3, L) bool)."""
	require_cuda(signal)
	N = signal.shape[1]
	ks = (int(kernel_size_smooth_silence), int(kernel_size_smooth_signal), int(kernel_size_smooth_speaker))
	L = _query('convasr_select_speaker_out_len', N, *ks)
	ws = workspace(_query('convasr_select_speaker_workspace_bytes', N, *ks), signal.device, 'diar')
	speaker_id = torch.empty(L, dtype = torch.float32, device = signal.device)
	mask = torch.empty(3, L, dtype = torch.bool, device = signal.device)
	call('convasr_select_speaker', ptr(signal), ptr(speaker_id), ptr(mask), ptr(ws), ws.numel(), N, *ks, float(silence_absolute_threshold), float(silence_relative_threshold),
	     float(eps), int(k), stream_ptr())
	return speaker_id, mask


def rle1d(x):
	"""Run-length encoding of a 1-D device tensor (convasr_rle1d_count / convasr_rle1d_write): (starts int64, lengths int64, values of x's
	dtype).  bool, integer and float32 inputs.  The number of runs decides the size of the result, so it is read back to the host ONCE between
	the two calls (4 bytes, one synchronisation)."""
	require_cuda(x)
	if x.ndim != 1 or x.numel() < 1:
		raise ValueError(f'rle1d: a 1-D tensor with at least one element expected, got shape {tuple(x.shape)}')
	if x.dtype != torch.float32 and (x.dtype.is_floating_point or x.dtype.is_complex):
		raise ValueError(f'rle1d: bool, integer and float32 tensors only, got {x.dtype}')
	n = x.numel()
	x = x.contiguous()
	kind = (x.element_size(), int(x.dtype == torch.float32))
	ws = workspace(_query('convasr_rle1d_workspace_bytes', n), x.device, 'rle')
	call('convasr_rle1d_count', ptr(x), *kind, n, ptr(ws), ws.numel(), stream_ptr())
	at = _query('convasr_rle1d_count_offset', n)
	runs = int(ws[at:at + 4].view(torch.int32).item()) + 1
	starts = torch.empty(runs, dtype = torch.int64, device = x.device)
	lengths = torch.empty(runs, dtype = torch.int64, device = x.device)
	values = torch.empty(runs, dtype = x.dtype, device = x.device)
	call('convasr_rle1d_write', ptr(x), *kind, n, ptr(ws), ws.numel(), runs, ptr(starts), ptr(lengths), ptr(values), stream_ptr())
	return starts, lengths, values


def speaker_error_counts(ref_mask, hyp_mask, perms):
	"""convasr_speaker_error_counts: ref_mask, hyp_mask (3, n) bool device tensors, perms a list of 3-element mappings.  Returns a
	(len(perms), 7) int64 device tensor: mismatches where exactly one reference speaker talks, mismatches anywhere, confusion, false alarm,
	miss, positions where exactly one reference speaker talks, positions where a reference speaker talks."""
	require_cuda(ref_mask, hyp_mask)
	if ref_mask.shape != hyp_mask.shape or ref_mask.ndim != 2 or ref_mask.shape[0] != 3 or ref_mask.dtype != torch.bool or hyp_mask.dtype != torch.bool:
		raise ValueError(f'speaker_error_counts: two (3, n) bool masks expected, got {tuple(ref_mask.shape)} {ref_mask.dtype} and {tuple(hyp_mask.shape)} {hyp_mask.dtype}')
	perms = [[int(v) for v in p] for p in perms]
	if not perms or any(len(p) != 3 for p in perms):
		raise ValueError('speaker_error_counts: mappings of 3 rows each expected')
	n = ref_mask.shape[1]
	ref_mask, hyp_mask = ref_mask.contiguous(), hyp_mask.contiguous()
	flat = (ctypes.c_int32 * (3 * len(perms)))(*[v for p in perms for v in p])
	ws = workspace(_query('convasr_speaker_error_counts_workspace_bytes', n), ref_mask.device, 'diar')
	counts = torch.empty(len(perms), 7, dtype = torch.int64, device = ref_mask.device)
	call('convasr_speaker_error_counts', ptr(ref_mask), ptr(hyp_mask), flat, len(perms), n, ptr(counts), ptr(ws), ws.numel(), stream_ptr())
	return counts


# ------------------------------------------------------------------------------------------------ audio

RESAMPLE_ZEROS, RESAMPLE_BETA, RESAMPLE_ROLLOFF = 64, 14.769656459379492, 0.9475937167399596  # the parameters resampy publishes for 'kaiser_best'
_resample_tables = {}  # (sr_in, sr_out, zeros, beta, rolloff) -> host table, (.., device) -> its copy there


def resample_tile():
	"""Outputs per workgroup of convasr_resample's tile route (tests straddle it)."""
	return _cached_query('convasr_resample_tile')


def resample_out_len(T_in, sr_in, sr_out):
	"""ceil(T_in * L / M), the length rule of include/convasr_hip.h (librosa's)."""
	return _query('convasr_resample_out_len', int(T_in), int(sr_in), int(sr_out))


def resample_table(sr_in, sr_out, zeros = RESAMPLE_ZEROS, beta = RESAMPLE_BETA, rolloff = RESAMPLE_ROLLOFF):
	"""The (taps, L) fp32 coefficient table of include/convasr_hip.h's resampler, computed in float64 on the host and rounded once; cached.
	Raises ConvasrHipError outside the envelope (L x taps > 2^22) before anything is computed."""
	import numpy as np
	key = (int(sr_in), int(sr_out), float(zeros), float(beta), float(rolloff))
	tab = _resample_tables.get(key)
	if tab is None:
		taps = _lib.call_rc('convasr_resample_taps', key[0], key[1], key[2], key[4])
		g = math.gcd(key[0], key[1])
		L, M = key[1] // g, key[0] // g
		s = key[4] * min(1.0, L / M)
		H = taps // 2 - 1
		d = (L * (np.arange(taps, dtype = np.int64)[:, None] - H) - np.arange(L, dtype = np.int64)[None, :]) / float(L)  # k - tau per (tap, phase)
		v = d * s / key[2]
		inside = np.abs(d) * s <= key[2]
		h = s * np.sinc(s * d) * np.i0(key[3] * np.sqrt(np.clip(1.0 - v * v, 0.0, None))) / np.i0(key[3])
		tab = _resample_tables[key] = torch.from_numpy(np.where(inside, h, 0.0).astype(np.float32))
	return tab


def resample(x, sr_in, sr_out, mono = False, zeros = RESAMPLE_ZEROS, beta = RESAMPLE_BETA, rolloff = RESAMPLE_ROLLOFF, route = 0):
	"""convasr_resample (include/convasr_hip.h): decode + de-interleave + optional mono mix + band-limited resampling in one launch.
	x: a device tensor, either (T, C) int16 -- interleaved PCM as a wav file holds it, scaled by 1 / 32767 -- or (C, T) float32.  Returns
	(C, T_out) float32, or (1, T_out) with mono, T_out = ceil(T * L / M).  sr_in == sr_out only decodes and mixes; T == 0 launches nothing.
	route: 0 automatic, 1 / 2 force the tile / direct kernel (tests; the result does not depend on it)."""
	require_cuda(x)
	if x.ndim != 2 or x.dtype not in (torch.int16, torch.float32):
		raise ValueError(f'resample: a (T, C) int16 or (C, T) float32 tensor expected, got {tuple(x.shape)} {x.dtype}')
	T, C = (x.shape[0], x.shape[1]) if x.dtype == torch.int16 else (x.shape[1], x.shape[0])
	sr_in, sr_out = int(sr_in), int(sr_out)
	table = None
	if sr_in != sr_out:
		key = (sr_in, sr_out, float(zeros), float(beta), float(rolloff), x.device)
		table = _resample_tables.get(key)
		if table is None:
			table = _resample_tables[key] = resample_table(sr_in, sr_out, zeros, beta, rolloff).to(x.device)
	T_out = resample_out_len(T, sr_in, sr_out)
	x = x.contiguous()
	out = torch.empty(1 if mono else C, T_out, dtype = torch.float32, device = x.device)
	call('convasr_resample', ptr(x), dtype_code(x.dtype), T, C, int(bool(mono)), ptr(table), 0 if table is None else table.shape[0], sr_in, sr_out, ptr(out), T_out, int(route), stream_ptr())
	return out


# ------------------------------------------------------------------------------------------------ speech activity, segments of a long recording

def frame_peak_tile(frame_len):
	"""Frames one workgroup of convasr_frame_peak takes per step at this frame length (tests straddle it)."""
	return _query('convasr_frame_peak_tile', int(frame_len))


def _vad_signal(name, signal):
	require_cuda(signal)
	if signal.ndim != 2 or signal.dtype not in (torch.int16, torch.float32):
		raise ValueError(f'{name}: a (C, N) int16 or float32 tensor expected, got {tuple(signal.shape)} {signal.dtype}')
	return signal.contiguous()


def _vad_frames_pair(name, mask, peaks):
	require_cuda(mask, peaks)
	if mask.ndim != 2 or mask.dtype != torch.bool or peaks.shape != mask.shape or peaks.dtype != torch.float32:
		raise ValueError(f'{name}: a (C, frames) bool mask and float32 peaks of the same shape expected, got {tuple(mask.shape)} {mask.dtype} and {tuple(peaks.shape)} {peaks.dtype}')
	return mask.contiguous(), peaks.contiguous()


def frame_peaks(signal, frame_len):
	"""convasr_frame_peak (include/convasr_hip.h): peak[c][f] = max |signal[c][f F : (f + 1) F]| of a (C, N) int16 or float32 device tensor, the
	last, partial frame included; int16 peaks are divided by 32767 once.  Returns (C, ceil(N / F)) float32.  One launch."""
	signal = _vad_signal('frame_peaks', signal)
	C, N = signal.shape
	F = int(frame_len)
	peaks = torch.empty(C, -(-N // F) if F > 0 else 0, dtype = torch.float32, device = signal.device)
	call('convasr_frame_peak', ptr(signal), dtype_code(signal.dtype), C, N, F, ptr(peaks), stream_ptr())
	return peaks


def vad_frames(peaks, n_full, abs_thr, rel_thr, eps, k, G, S, P):
	"""The raw and the smoothed speech mask of include/convasr_hip.h from frame peaks (C, nF): level = the k-th smallest (1-based) of the first
	n_full peaks of every channel (kth_value), raw = the threshold test on whole frames, mask = raw after the three smoothing steps of G, S, P
	frames (convasr_vad_frames, one launch).  Returns (raw, mask), (C, nF) bool.  n_full == 0: both all False, nothing is launched."""
	require_cuda(peaks)
	if peaks.ndim != 2 or peaks.dtype != torch.float32:
		raise ValueError(f'vad_frames: peaks must be a (C, frames) float32 tensor, got {tuple(peaks.shape)} {peaks.dtype}')
	C, nF = peaks.shape
	n_full = int(n_full)
	if n_full == 0:
		return torch.zeros(C, nF, dtype = torch.bool, device = peaks.device), torch.zeros(C, nF, dtype = torch.bool, device = peaks.device)
	peaks = peaks.contiguous()
	level = kth_value(peaks[:, :n_full], k)
	raw = torch.empty(C, nF, dtype = torch.bool, device = peaks.device)
	mask = torch.empty(C, nF, dtype = torch.bool, device = peaks.device)
	ws = workspace(_query('convasr_vad_frames_workspace_bytes', C, nF), peaks.device, 'vad')
	call('convasr_vad_frames', ptr(peaks), ptr(level), C, nF, n_full, float(abs_thr), float(rel_thr), float(eps), int(G), int(S), int(P), ptr(raw), ptr(mask), ptr(ws), ws.numel(), stream_ptr())
	return raw, mask


def vad_segments(mask, peaks, frame_len, N, max_frames):
	"""The speech runs of a (C, nF) bool mask over a recording of N samples in frames of frame_len, cut at their quietest frames (peaks) into
	pieces of at most max_frames frames (0: no cutting) -- include/convasr_hip.h.  Returns (channel, first, count): int64 device tensors, one
	entry per segment, by channel and then time, first and count in samples.  The number of segments decides the size of the result, so it is
	read back to the host ONCE between the two calls (convasr_vad_segments_count / _write), as in rle1d."""
	mask, peaks = _vad_frames_pair('vad_segments', mask, peaks)
	C, nF = mask.shape
	ws = workspace(_query('convasr_vad_segments_workspace_bytes', C, nF), mask.device, 'vad')
	call('convasr_vad_segments_count', ptr(mask), ptr(peaks), C, nF, int(max_frames), ptr(ws), ws.numel(), stream_ptr())
	total = int(ws[:4 * C].view(torch.int32).sum().item())
	channel, first, count = (torch.empty(total, dtype = torch.int64, device = mask.device) for _ in range(3))
	if total > 0:
		call('convasr_vad_segments_write', ptr(mask), C, nF, int(frame_len), int(N), ptr(ws), ws.numel(), total, ptr(channel), ptr(first), ptr(count), stream_ptr())
	return channel, first, count


def gather_segments(signal, channel, first, count, multiple = 128):
	"""convasr_gather_segments: the segments (channel_b, first_b, count_b) -- tensors or lists of B integers, on either side -- of a (C, N) int16
	or float32 device signal as one zero-padded float32 batch, in one launch.  Returns (x (B, Tpad), xlen (B,) float32 = count / Tpad) with
	Tpad = ceil(max count / multiple) * multiple, AudioTextDataset.collate_fn's rule.  The library checks a host copy of the segments against
	the signal before the launch: a segment that leaves [0, N) raises ConvasrHipError."""
	signal = _vad_signal('gather_segments', signal)
	C, N = signal.shape
	rows = [torch.as_tensor(r, dtype = torch.int64).reshape(-1) for r in (channel, first, count)]
	B = rows[0].numel()
	if B < 1 or any(r.numel() != B for r in rows) or int(multiple) < 1:
		raise ValueError(f'gather_segments: three lists of one length >= 1 and a multiple >= 1 expected, got {[r.numel() for r in rows]} and {multiple}')
	host = torch.stack([r.cpu() for r in rows]).contiguous()
	seg = torch.stack(rows).contiguous() if all(r.device == signal.device for r in rows) else host.to(signal.device)
	longest = int(host[2].max())
	Tpad = max(int(math.ceil(longest / int(multiple))) * int(multiple), 1)
	x = torch.empty(B, Tpad if longest <= N else 0, dtype = torch.float32, device = signal.device)  # (a count beyond the signal: the library refuses it below, nothing that large is allocated)
	call('convasr_gather_segments', ptr(signal), dtype_code(signal.dtype), C, N, host.data_ptr(), ptr(seg), B, ptr(x), Tpad, stream_ptr())
	xlen = torch.tensor([l / Tpad for l in host[2].tolist()], dtype = torch.float32).to(signal.device, non_blocking = True)
	return x, xlen


# ------------------------------------------------------------------------------------------------ training-time augmentation (the project's own, unpinned: include/convasr_hip.h)

AUG_ONE = 1 << 32  # speed 1.0 in the 32.32 fixed point of convasr_augment_params
AUG_FIELDS = ('speed', 'step', 'gain', 'noise_row', 'noise_offset', 'snr', 'len', 'out_len')  # the columns of the (B, 8) parameter tensor


def philox(counters, key):
	"""convasr_philox: the raw Philox4x32-10 blocks of the augmentation generator.  counters (N, 4) int64 holding 32-bit words on the device,
	key two 32-bit words.  Returns (N, 4) int64, the four output words of every block."""
	require_cuda(counters)
	if counters.ndim != 2 or counters.shape[1] != 4 or counters.dtype != torch.int64:
		raise ValueError(f'philox: (N, 4) int64 counters expected, got {tuple(counters.shape)} {counters.dtype}')
	counters = counters.contiguous()
	out = torch.empty_like(counters)
	call('convasr_philox', ptr(counters), counters.shape[0], int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff, ptr(out), stream_ptr())
	return out


def augment_tile():
	"""Outputs per tile of convasr_augment_waveform (tests straddle it)."""
	return _cached_query('convasr_augment_tile')


def augment_phases():
	"""Tabulated phases per input sample of the speed filter."""
	return _cached_query('convasr_augment_phases')


def prob_threshold(p):
	"""floor(p * 2^24): a draw fires when its top 24 bits are below it."""
	if not 0.0 <= float(p) <= 1.0:
		raise ValueError(f'a probability in [0, 1] expected, got {p}')
	return int(math.floor(float(p) * (1 << 24)))


def augment_steps(speeds):
	"""round(speed * 2^32) per speed, the fixed-point steps of include/convasr_hip.h (halves round up; speed * 2^32 is exact in float64)."""
	return [int(math.floor(float(s) * AUG_ONE + 0.5)) for s in speeds]


def augment_table(steps, zeros = RESAMPLE_ZEROS, beta = RESAMPLE_BETA, rolloff = RESAMPLE_ROLLOFF):
	"""The (n_speeds, taps, phases + 1) fp32 filter table of convasr_augment_waveform, computed in float64 on the host and rounded once, and its
	taps.  (None, 0) when every speed is 1.0: nothing is filtered."""
	import numpy as np
	if all(s == AUG_ONE for s in steps):
		return None, 0
	P = augment_phases()
	cut = [float(rolloff) * min(1.0, AUG_ONE / s) for s in steps]
	H = int(math.floor(float(zeros) / min(cut)))
	taps = 2 * H + 2
	d = (np.arange(taps, dtype = np.float64)[:, None] - H) - np.arange(P + 1, dtype = np.float64)[None, :] / P
	tab = np.zeros((len(steps), taps, P + 1), dtype = np.float32)
	for i, c in enumerate(cut):
		v = d * c / float(zeros)
		h = c * np.sinc(c * d) * np.i0(float(beta) * np.sqrt(np.clip(1.0 - v * v, 0.0, None))) / np.i0(float(beta))
		tab[i] = np.where(np.abs(d) * c <= float(zeros), h, 0.0).astype(np.float32)
	return torch.from_numpy(tab), taps


def db_table(lo_db, hi_db, steps, sign = 1.0):
	"""`steps` values 10^(sign * dB / 20), dB evenly spaced from lo_db to hi_db (one step: lo_db), in float64, rounded once to fp32."""
	import numpy as np
	db = np.linspace(float(lo_db), float(hi_db), int(steps), dtype = np.float64) if int(steps) > 1 else np.full(int(steps), float(lo_db), dtype = np.float64)
	return torch.from_numpy((10.0 ** (sign * db / 20.0)).astype(np.float32))


def _augment_batch(name, x):
	require_cuda(x)
	if x.ndim != 2 or x.dtype not in (torch.int16, torch.float32):
		raise ValueError(f'{name}: a (B, T) int16 or float32 batch expected, got {tuple(x.shape)} {x.dtype}')
	if x.shape[1] >= 1 << 31:
		raise _lib.ConvasrHipError(f'{name}: T {x.shape[1]} >= 2^31')
	return x.contiguous()


def _same_device(name, dev, **tensors):
	for what, t in tensors.items():
		if t is not None and t.device != dev:
			raise _lib.ConvasrHipError(f'{name}: {what} lives on {t.device}, the batch on {dev}')


def augment_params(xlen, keys, T, seed, epoch, steps, speed_thr = 1 << 24, gain_steps = 0, gain_thr = 0, noise_shape = None, snr_steps = 1, noise_thr = 0, min_out_len = None):
	"""convasr_augment_params: every random decision of the waveform augmentation as integers.  xlen (B,) float32 fractions of T, keys (B,) int64,
	steps a list of fixed-point speeds (augment_steps), the thresholds from prob_threshold, noise_shape = (rows, samples) of the noise bank or
	None.  Returns (params (B, 8) int64 with the columns AUG_FIELDS, xlen_out (B,) float32 = out_len / T).  One launch; B == 0 or T == 0: none."""
	require_cuda(xlen, keys)
	dev = xlen.device
	B, T = xlen.shape[0], int(T)
	_same_device('augment_params', dev, keys = keys, min_out_len = min_out_len)
	if keys.shape != (B,) or keys.dtype != torch.int64 or (min_out_len is not None and (min_out_len.shape != (B,) or min_out_len.dtype != torch.int64)):
		raise ValueError(f'augment_params: keys and min_out_len must be ({B},) int64 tensors')
	xlen, keys = xlen_f32(xlen, dev), keys.contiguous()
	min_out_len = None if min_out_len is None else min_out_len.contiguous()
	rows, samples = (0, 0) if noise_shape is None else (int(noise_shape[0]), int(noise_shape[1]))
	params = torch.zeros(B, len(AUG_FIELDS), dtype = torch.int64, device = dev) if B == 0 or T == 0 else torch.empty(B, len(AUG_FIELDS), dtype = torch.int64, device = dev)
	xlen_out = xlen.clone() if B == 0 or T == 0 else torch.empty(B, dtype = torch.float32, device = dev)
	arr = (ctypes.c_uint64 * max(len(steps), 1))(*[int(s) for s in steps])
	call('convasr_augment_params', ptr(xlen), ptr(keys), ptr(min_out_len), B, T, int(seed) & 0xffffffffffffffff, int(epoch), arr, len(steps), int(speed_thr), int(gain_steps), int(gain_thr),
	     rows, samples, int(snr_steps), int(noise_thr), ptr(params), ptr(xlen_out), stream_ptr())
	return params, xlen_out


def reverb_block():
	"""Outputs per block Bk of convasr_augment_reverb's partitioned convolution; its FFTs have 2 Bk points (tests straddle it)."""
	return _cached_query('convasr_augment_reverb_block')


def reverb_direct():
	"""min(rir_len, out_len) up to which convasr_augment_reverb sums an utterance's products directly instead of through FFTs."""
	return _cached_query('convasr_augment_reverb_direct')


_reverb_twiddles = {}


def reverb_twiddles(device):
	"""The (Bk, 4) fp32 table (c_hi, s_hi, c_lo, s_lo) of convasr_augment_reverb on `device`, c = cos(pi t / Bk), s = -sin(pi t / Bk): float64 on the
	host, each split once into its fp32 rounding and the fp32 remainder, kept."""
	import numpy as np
	t = _reverb_twiddles.get(device)
	if t is None:
		a = np.pi * np.arange(reverb_block(), dtype = np.float64) / reverb_block()
		w = np.stack([np.cos(a), -np.sin(a)], axis = 1)
		hi = w.astype(np.float32)
		t = _reverb_twiddles[device] = torch.from_numpy(np.concatenate([hi, (w - hi.astype(np.float64)).astype(np.float32)], axis = 1)).to(device)
	return t


def rir_delays(rir, rir_len):
	"""d_r, the index of the first largest |h_r[k]| over k < rir_len[r] (the direct path): (R,) int64 on the CPU.  Host work, done once per bank."""
	h = rir.detach().cpu().abs()
	n = torch.as_tensor(rir_len, dtype = torch.int64).cpu()
	return torch.tensor([int(h[r, :max(int(n[r]), 1)].argmax()) for r in range(h.shape[0])], dtype = torch.int64)


def reverb_params(keys, seed, epoch, rir_rows, reverb_thr):
	"""convasr_augment_reverb_params: rir_row (B,) int64, the row of the bank of rir_rows impulse responses each utterance is convolved with, -1
	= none (purposes 12 and 13 of the generator; reverb_thr from prob_threshold).  One launch; B == 0: none."""
	require_cuda(keys)
	if keys.ndim != 1 or keys.dtype != torch.int64:
		raise ValueError(f'reverb_params: keys must be a (B,) int64 tensor, got {tuple(keys.shape)} {keys.dtype}')
	keys = keys.contiguous()
	rir_row = torch.empty(keys.shape[0], dtype = torch.int64, device = keys.device)
	call('convasr_augment_reverb_params', ptr(keys), keys.shape[0], int(seed) & 0xffffffffffffffff, int(epoch), int(rir_rows), int(reverb_thr), ptr(rir_row), stream_ptr())
	return rir_row


def augment_reverb(y, params, rir_row, rir, rir_len, rir_delay, noise = None, host = None):
	"""convasr_augment_reverb: y (B, T) float32, the output of the speed and gain pass, convolved per utterance with row rir_row[b] of the bank
	rir (R, Lmax) float32, shifted by the row's direct-path delay and cut at out_len -> (out (B, T) float32, partials (B, parts, 2) float64, the
	energies of the result and of the noise window that convasr_augment_mix reads; a view of a workspace, valid until the next call).  rir_len,
	rir_delay: (R,) int64 device tensors; host: their (rir_len, rir_delay) copies as CPU int64 tensors, which the argument checks read -- None
	copies them back from the device, which synchronises.  Three launches; B == 0 or T == 0 launches nothing."""
	require_cuda(y, params, rir_row, rir, rir_len, rir_delay, noise)
	if y.ndim != 2 or y.dtype != torch.float32:
		raise ValueError(f'augment_reverb: a (B, T) float32 batch expected, got {tuple(y.shape)} {y.dtype}')
	dev = y.device
	B, T = y.shape
	_same_device('augment_reverb', dev, params = params, rir_row = rir_row, rir = rir, rir_len = rir_len, rir_delay = rir_delay, noise = noise)
	if params.shape != (B, len(AUG_FIELDS)) or params.dtype != torch.int64 or rir_row.shape != (B,) or rir_row.dtype != torch.int64:
		raise ValueError(f'augment_reverb: params must be ({B}, {len(AUG_FIELDS)}) int64 and rir_row ({B},) int64, got {tuple(params.shape)} {params.dtype} and {tuple(rir_row.shape)} {rir_row.dtype}')
	if rir.ndim != 2 or rir.dtype != torch.float32 or (noise is not None and (noise.ndim != 2 or noise.dtype != torch.float32)):
		raise ValueError(f'augment_reverb: the bank must be a (R, Lmax) float32 tensor (the noise a (N, L) one), got {tuple(rir.shape)} {rir.dtype}')
	R, Lmax = rir.shape
	if host is None:
		host = (rir_len.cpu(), rir_delay.cpu())
	for what, t in (('rir_len', rir_len), ('rir_delay', rir_delay), ('host rir_len', host[0]), ('host rir_delay', host[1])):
		if t.shape != (R,) or t.dtype != torch.int64:
			raise ValueError(f'augment_reverb: {what} must be a ({R},) int64 tensor, got {tuple(t.shape)} {t.dtype}')
	if host[0].is_cuda or host[1].is_cuda:
		raise ValueError('augment_reverb: host = (rir_len, rir_delay) must be CPU tensors')
	y, params, rir_row, rir, rir_len, rir_delay = (t.contiguous() for t in (y, params, rir_row, rir, rir_len, rir_delay))
	len_host, delay_host = host[0].contiguous(), host[1].contiguous()
	noise = None if noise is None else noise.contiguous()
	parts = _cached_query('convasr_augment_parts')
	out = torch.empty(B, T, dtype = torch.float32, device = dev)
	partials = workspace(max(B, 1) * parts * 16, dev, 'augment')
	longest = int(len_host.max()) if R > 0 else 0
	nbytes = _cached_query('convasr_augment_reverb_workspace_bytes', B, T, longest)
	ws = workspace(nbytes, dev, 'reverb')
	rows, samples = (0, 0) if noise is None else noise.shape
	call('convasr_augment_reverb', ptr(y), B, T, ptr(params), ptr(rir_row), ptr(rir), R, Lmax, ptr(rir_len), ptr(rir_delay), ptr(len_host), ptr(delay_host), ptr(reverb_twiddles(dev)), ptr(noise),
	     rows, samples, ptr(out), ptr(partials), ptr(ws), ws.numel(), stream_ptr())
	return out, partials[:B * parts * 16].view(torch.float64).view(B, parts, 2)


def augment_waveform(x, params, table = None, gain_table = None, noise = None, snr_table = None, rir = None, rir_len = None, rir_delay = None, rir_row = None, rir_host = None):
	"""convasr_augment_waveform + convasr_augment_mix: x (B, T) float32 or int16 (scaled by 1 / 32767) -> (out (B, T) float32 of the same padded
	length, scales (B,) float32, the factor each utterance's noise was added with; 0 = none).  params: augment_params' tensor; table
	(n_speeds, taps, phases + 1), gain_table, noise (N, L) and snr_table float32 device tensors (None: no speeds other than 1.0 / no gain / no
	noise).  Two launches, a third with a noise bank; B == 0 or T == 0 launches nothing.
	With a bank of room impulse responses -- rir (R, Lmax) float32, rir_len and rir_delay (R,) int64, rir_row (B,) int64 from reverb_params,
	rir_host as augment_reverb's `host` -- convasr_augment_reverb runs between the two (three more launches) and the noise is mixed at an SNR
	relative to the reverberated speech; without one, nothing changes."""
	x = _augment_batch('augment_waveform', x)
	dev = x.device
	B, T = x.shape
	_same_device('augment_waveform', dev, params = params, table = table, gain_table = gain_table, noise = noise, snr_table = snr_table)
	if params.shape != (B, len(AUG_FIELDS)) or params.dtype != torch.int64:
		raise ValueError(f'augment_waveform: params must be ({B}, {len(AUG_FIELDS)}) int64, got {tuple(params.shape)} {params.dtype}')
	for what, t, nd in (('table', table, 3), ('gain_table', gain_table, 1), ('noise', noise, 2), ('snr_table', snr_table, 1)):
		if t is not None and (t.ndim != nd or t.dtype != torch.float32):
			raise ValueError(f'augment_waveform: {what} must be a {nd}-d float32 tensor, got {tuple(t.shape)} {t.dtype}')
	if table is not None and table.shape[2] != augment_phases() + 1:
		raise ValueError(f'augment_waveform: a table of {augment_phases() + 1} columns expected, got {tuple(table.shape)}')
	if noise is not None and snr_table is None:
		raise ValueError('augment_waveform: a noise bank needs an SNR table')
	if rir is not None and (rir_len is None or rir_delay is None or rir_row is None):
		raise ValueError('augment_waveform: a bank of impulse responses needs rir_len, rir_delay and rir_row')
	params, table, gain_table, noise, snr_table = (None if t is None else t.contiguous() for t in (params, table, gain_table, noise, snr_table))
	out = torch.empty(B, T, dtype = torch.float32, device = dev)
	scales = torch.zeros(B, dtype = torch.float32, device = dev) if noise is None or B == 0 or T == 0 else torch.empty(B, dtype = torch.float32, device = dev)
	ws = workspace(max(B, 1) * _cached_query('convasr_augment_parts') * 16, dev, 'augment')
	rows, samples = (0, 0) if noise is None else noise.shape
	call('convasr_augment_waveform', ptr(x), dtype_code(x.dtype), B, T, ptr(params), ptr(table), 0 if table is None else table.shape[0], 0 if table is None else table.shape[1], ptr(gain_table),
	     0 if gain_table is None else gain_table.numel(), ptr(noise), rows, samples, ptr(out), ptr(ws), stream_ptr())
	if rir is not None:
		out, partials = augment_reverb(out, params, rir_row, rir, rir_len, rir_delay, noise, rir_host)  # (the partials are the same workspace, rewritten)
		ws = partials
	if noise is not None:
		call('convasr_augment_mix', ptr(out), B, T, ptr(params), ptr(noise), rows, samples, ptr(snr_table), snr_table.numel(), ptr(ws), ptr(scales), stream_ptr())
	return out, scales


def spec_augment_tile():
	"""Elements one workgroup of convasr_spec_augment takes per step (tests straddle it)."""
	return _cached_query('convasr_spec_augment_tile')


def spec_augment(x, xlen, keys, epoch, seed, freq_masks = 2, freq_width = 10, time_masks = 2, time_width = 50, time_fraction = 0.05, fill = 'mean', return_masks = False):
	"""convasr_spec_augment: frequency and time masks on (B, F, T) float32 features, one launch.  xlen (B,) float32 fractions of T; keys (>= B,)
	int64 and epoch (1,) int64 are DEVICE tensors the kernel reads, so a captured graph draws fresh masks from rewritten buffers.  fill: a number,
	or 'mean' = each utterance's mean over all channels and valid frames.  Returns (out, fill (B,) float32) and, with return_masks, the
	(B, freq_masks + time_masks, 2) int32 (start, width) pairs, frequency masks first."""
	require_cuda(x, xlen, keys, epoch)
	if x.ndim != 3 or x.dtype != torch.float32:
		raise ValueError(f'spec_augment: (B, F, T) float32 features expected, got {tuple(x.shape)} {x.dtype}')
	B, F, T = x.shape
	dev = x.device
	_same_device('spec_augment', dev, xlen = xlen, keys = keys, epoch = epoch)
	if keys.ndim != 1 or keys.shape[0] < B or keys.dtype != torch.int64 or not keys.is_contiguous() or epoch.dtype != torch.int64 or epoch.numel() != 1:
		raise ValueError(f'spec_augment: keys must be a contiguous int64 tensor of at least {B} entries and epoch one int64, got {tuple(keys.shape)} {keys.dtype} and {tuple(epoch.shape)} {epoch.dtype}')
	x, xlen = x.contiguous(), xlen_f32(xlen, dev)
	mean = fill == 'mean'
	out = torch.empty_like(x)
	fill_out = torch.zeros(B, dtype = torch.float32, device = dev) if B * F * T == 0 else torch.empty(B, dtype = torch.float32, device = dev)
	masks = torch.zeros(B, int(freq_masks) + int(time_masks), 2, dtype = torch.int32, device = dev) if return_masks else None
	call('convasr_spec_augment', ptr(x), ptr(xlen), ptr(keys), ptr(epoch), int(seed) & 0xffffffffffffffff, B, F, T, int(freq_masks), int(freq_width), int(time_masks), int(time_width),
	     prob_threshold(time_fraction), int(mean), 0.0 if mean else float(fill), ptr(out), ptr(fill_out), ptr(masks), stream_ptr())
	return (out, fill_out, masks) if return_masks else (out, fill_out)
