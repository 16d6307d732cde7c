"""Float64 numpy restatements of the two distillation rules of include/convasr_hip.h -- convasr_topk_frames (the order on (value, class)
pairs, ties and NaNs included) and convasr_distill_kl (the KL of a truncated, renormalised teacher against a student, with the gradient)
-- and the inputs the GPU tests feed both (tests/test_distill_gpu.py), so that tests/test_distill_ref.py can hold a float32 copy of the
restatement to the GPU tests' bars on the very same arrays.

Arrays are (B, T, C) / (B, T, k): the memory layout of the kernels (the ops hand out (B, C, T) / (B, k, T) views of it)."""
import numpy as np

U = 2.0 ** -24
KD_BAR = (1e-4, 1e-5)    # per-frame tau^2 KL and kd[b] (atol x the utterance's frames): the project's entropy bar
GRAD_BAR = (1e-4, 1e-5)  # x tau: the project's log-softmax-backward bar
B = 3
FRAMES = (1, 127, 128, 129, 300)       # around the 128-frame workgroup of the row mapping
CLASSES = (2, 38, 64, 65, 130, 512)    # both sides of the mapping switch at 64, a class count that is no multiple of 64
TAUS = (0.5, 1.0, 2.0)


# ------------------------------------------------------------------------------------------------ top-k

def order(x):
	"""The classes of every frame in the rule's total order: a NaN above every number, larger values first, equal values (-0.0 == 0.0) and
	NaNs among themselves by the lower class."""
	x = np.asarray(x, dtype = np.float64)
	nan = np.isnan(x)
	cls = np.broadcast_to(np.arange(x.shape[-1]), x.shape)
	return np.lexsort((cls, np.where(nan, 0.0, -x), ~nan), axis = -1)  # the last key is the primary one; ties fall to the key before it


def topk(x, k):
	"""(values, indices) (..., k): values keep x's dtype and bits."""
	idx = order(x)[..., :k]
	return np.take_along_axis(np.asarray(x), idx, axis = -1), idx.astype(np.int64)


# ------------------------------------------------------------------------------------------------ KL and gradient

def distill(z, values, indices, lengths, tau, dtype = np.float64):
	"""(kd (B,), kd_frames (B, T), grad (B, T, C)) of the rule, every step in `dtype` (float64: the reference; float32: a copy that shows
	what fp32 arithmetic can hold).  The direct form sum_j p_j (log p_j - log q[idx_j]), not the kernel's rearrangement."""
	z, v = np.asarray(z).astype(dtype), np.asarray(values).astype(dtype)
	idx = np.asarray(indices).astype(np.int64)
	Bz, T, C = z.shape
	it, tau_d = dtype(1.0) / dtype(tau), dtype(tau)
	with np.errstate(all = 'ignore'):
		s = z * it
		s = s - s.max(-1, keepdims = True)
		logq = s - np.log(np.exp(s).sum(-1, keepdims = True, dtype = dtype))
		u = v * it
		u = u - u.max(-1, keepdims = True)
		e = np.exp(u)
		Sp = e.sum(-1, keepdims = True, dtype = dtype)
		p, logp = e / Sp, u - np.log(Sp)
		bad = ((idx < 0) | (idx >= C)).any(-1)
		idc = np.clip(idx, 0, C - 1)
		frames = tau_d * tau_d * (p * (logp - np.take_along_axis(logq, idc, axis = -1))).sum(-1, dtype = dtype)
		grad = tau_d * np.exp(logq)
		bi, ti = np.meshgrid(np.arange(Bz), np.arange(T), indexing = 'ij')
		for j in range(idx.shape[-1]):
			np.subtract.at(grad, (bi, ti, idc[..., j]), tau_d * p[..., j])
	frames[bad] = np.nan
	grad[bad] = np.nan
	n = np.clip(np.asarray(lengths, dtype = np.int64), 0, T)
	dead = np.arange(T)[None, :] >= n[:, None]
	frames[dead] = 0
	grad[dead] = 0
	kd = np.array([frames[b, :n[b]].sum(dtype = np.float64) for b in range(Bz)]).astype(dtype)
	return kd, frames, grad


def dense_teacher(values, indices, C, tau):
	"""softmax(values / tau) over the kept classes, scattered to C classes (float64): the p_dense of the autograd checks."""
	u = np.asarray(values, dtype = np.float64) / tau
	e = np.exp(u - u.max(-1, keepdims = True))
	p = e / e.sum(-1, keepdims = True)
	dense = np.zeros(u.shape[:-1] + (C, ))
	np.put_along_axis(dense, np.asarray(indices, dtype = np.int64), p, axis = -1)
	return dense


def share(got, want, rtol, atol):
	"""The worst |got - want| / (atol + rtol |want|) over the entries (NaN positions must agree); atol may be an array."""
	got, want = np.asarray(got, dtype = np.float64), np.asarray(want, dtype = np.float64)
	assert got.shape == want.shape, (got.shape, want.shape)
	assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions differ'
	ok = ~np.isnan(want)
	if not ok.any():
		return 0.0
	bar = np.broadcast_to(atol + rtol * np.abs(want), want.shape)
	return float((np.abs(got - want)[ok] / bar[ok]).max())


def held(name, got, want, rtol, atol):
	"""share() printed next to its bar, and asserted to be at most 1."""
	use = share(got, want, rtol, atol)
	print(f'  {name}: {use:.3f} of its bar (rtol {rtol:g}, atol {float(np.max(atol)):.3g})')
	assert use <= 1.0, (name, use)
	return use


def check_distill(name, got, want, lengths, tau, T):
	"""(kd, kd_frames, grad) against the float64 restatement's, on the bars of the module's head."""
	n = np.clip(np.asarray(lengths, dtype = np.float64), 0, T)
	return max(held(name + ' kd', got[0], want[0], KD_BAR[0], KD_BAR[1] * np.maximum(n, 1.0)),
	           held(name + ' kd_frames', got[1], want[1], *KD_BAR),
	           held(name + ' grad', got[2], want[2], GRAD_BAR[0], tau * GRAD_BAR[1]))


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests

def lengths_of(T):
	return [[0, 1, T], [T - 1, T, 0]]  # {0, 1, T - 1, T} across the two batches of three


def topk_inputs(C, T):
	"""name -> (B, T, C) float32 logits; TIE_FREE names those torch.topk must agree with in the indices too."""
	rng = np.random.default_rng(7000 * C + T)
	x = {'normal x 3': (rng.standard_normal((B, T, C)) * 3).astype(np.float32)}
	x['tied integers'] = rng.integers(-3, 4, (B, T, C)).astype(np.float32)
	x['tied integers'][0, 0, :2] = [0.0, -0.0]  # -0.0 == 0.0: the lower class first
	one = x['normal x 3'].copy()
	one[np.arange(B), rng.integers(0, T, B), rng.integers(0, C, B)] = np.nan
	x['one NaN'] = one
	several = x['tied integers'].copy()
	several[rng.random((B, T, C)) < 0.3] = np.nan
	several[0, 0] = np.nan  # a frame of nothing but NaNs
	x['several NaNs'] = several
	x['+-80'] = np.where(rng.random((B, T, C)) < 0.5, 80.0, -80.0).astype(np.float32)
	base = ((np.arange(C) - C / 2) * 0.37).astype(np.float32)  # distinct values, permuted per frame: no ties, whatever C is
	x['permutation'] = rng.permuted(np.tile(base, (B, T, 1)), axis = -1)
	return x


TIE_FREE = ('permutation', )


def distill_students(C, T):
	rng = np.random.default_rng(9000 * C + T)
	z80 = np.where(rng.random((B, T, C)) < 0.5, 80.0, -80.0).astype(np.float32)
	return {'normal x 3': (rng.standard_normal((B, T, C)) * 3).astype(np.float32), '+-80': z80}


def distill_teacher_logits(C, T):
	return (np.random.default_rng(11000 * C + T).standard_normal((B, T, C)) * 3).astype(np.float32)


def distill_settings(C):
	"""(k, tau, values dtype, indices dtype): k x tau in full with fp32 / int32 storage, every other storage type at k = 8, tau = 2."""
	ks = sorted({1, min(8, C)})
	out = [(k, tau, 'float32', 'int32') for k in ks for tau in TAUS]
	out += [(ks[-1], 2.0, v, i) for v in ('float32', 'float16') for i in (('uint8', ) if C <= 256 else ()) + ('int16', 'int32') if (v, i) != ('float32', 'int32')]
	return out
