"""Float64 numpy restatement of convasr_ema_update (include/convasr_hip.h has the rule and the order of operations), the weight average
train.WeightEMA keeps: the warm-up schedule, the skip rule and the 16-bit mirror.

The decay d = min(decay, (1 + k) / (10 + k)) and 1 - d are taken in fp32, in the kernel's order (two sums, one quotient, one difference, each
correctly rounded) -- they are the launch's scalars, the same for every element; the element update e + (1 - d) (w - e) is float64.  The
kernel rounds the difference and the fused multiply-add, at most 2^-24 relative to the larger operand each: m updates may differ from this
restatement by m 2^-23 max(|w|, |e|) per element (tests/test_ema_gpu.py)."""
import numpy as np

F32 = np.float32
LS_OVERFLOW = 2  # include/convasr_hip.h: field [2] of the loss scaler's state, "did the last step overflow"
K_MAX = 2.0 ** 24  # the device counter is a float and saturates here


def schedule(decay, k):
	"""(d, 1 - d) as fp32 values for update number k (k updates applied so far)."""
	k = F32(k)
	d = min(F32(decay), (F32(1) + k) / (F32(10) + k))
	return F32(d), F32(F32(1) - F32(d))


def skipped(loss_gate = None, scaler_state = None):
	"""The optimizers' rule: a non-finite gate, or an overflow recorded in the scaler state the step wrote."""
	gated = loss_gate is not None and not (abs(float(loss_gate)) < float('inf'))
	return bool(gated or (scaler_state is not None and float(scaler_state[LS_OVERFLOW]) != 0.0))


def update(w, e, k, decay, loss_gate = None, scaler_state = None):
	"""One update: (e', k').  w: the parameters (fp32 values, any float array), e: the average so far (float64), k: updates applied so far."""
	w, e = np.asarray(w, dtype = np.float64), np.asarray(e, dtype = np.float64)
	if skipped(loss_gate, scaler_state):
		return e.copy(), k
	if k == 0:
		return w.copy(), 1
	_, omd = schedule(decay, k)
	return e + np.float64(omd) * (w - e), int(min(k + 1, K_MAX))


def round_bf16(x):
	"""fp32 -> bf16 bits (uint16), round-to-nearest-even; NaN stays a NaN."""
	u = np.ascontiguousarray(x, dtype = F32).view(np.uint32).astype(np.uint64)
	r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
	nan = np.isnan(np.asarray(x, dtype = F32))
	return np.where(nan, np.uint16(0x7fc0), r)


def round_f16(x):
	"""fp32 -> fp16 bits (uint16), round-to-nearest-even, +-inf beyond 65504."""
	with np.errstate(over = 'ignore'):
		return np.ascontiguousarray(x, dtype = F32).astype(np.float16).view(np.uint16)


def mirror_bits(e32, dtype):
	"""The expected 16-bit mirror of an fp32 average, as uint16 bit patterns; dtype 'bf16' or 'f16'."""
	return dict(bf16 = round_bf16, f16 = round_f16)[dtype](e32)
