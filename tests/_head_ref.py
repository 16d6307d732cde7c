"""float64 restatement of the log-prob head and the plumbing kernels (convasr_amd/csrc/misc.hip, collate_pad of csrc/next.hip, signal_absmax
of csrc/frontend.hip), plain torch / numpy on the CPU.  Nothing here loads the library.

Activations are LOGICAL (B, C, T) tensors, the class / channel axis is dim 1 -- the convention of convasr_amd.ops and of the oracle.  Every
function takes the values exactly as the kernel receives them (fp32, or the 16-bit / int16 storage values) and returns what the operation
means mathematically, in float64.  The exact ops (permutations, copies, one round-to-nearest-even into the storage type, ceil of an fp32
product) are expressed with torch's own casts and fp32 arithmetic instead: they have one right answer, bit for bit.
tests/test_head_ref.py holds all of this to torch's float64 ops, the oracle and the committed goldens."""
import numpy as np
import torch


def f64(t):
	return None if t is None else t.detach().to(device = 'cpu', dtype = torch.float64)


# ------------------------------------------------------------------------------------------------ log-softmax

def log_softmax(logits):
	"""x - logsumexp(x) over the class axis; a -inf logit has probability 0 and log-probability -inf"""
	x = f64(logits)
	m = x.max(dim = 1, keepdim = True).values
	return x - m - (x - m).exp().sum(dim = 1, keepdim = True).log()


def log_softmax_bwd(grad_lp, log_probs):
	"""d / d logits of sum(grad_lp * log_softmax(logits)) = g - softmax * sum_c g"""
	g, lp = f64(grad_lp), f64(log_probs)
	return g - lp.exp() * g.sum(dim = 1, keepdim = True)


# ------------------------------------------------------------------------------------------------ entropies (oracle/convasr_oracle.py:519-534)

def frame_mask(T, lengths):
	"""(B, T) float64: 1 where t < lengths[b]"""
	return (torch.arange(T).unsqueeze(0) < lengths.detach().cpu().long().unsqueeze(1)).to(torch.float64)


def frame_entropy(log_probs):
	lp = f64(log_probs)
	return -(lp.exp() * lp).sum(dim = 1)


def entropy(log_probs, olen = None, eps = 1e-9):
	"""mean over all T frames (olen None) or sum over the frames t < olen[b] / (eps + olen[b]); olen may exceed T (the divisor follows olen)"""
	e = frame_entropy(log_probs)
	if olen is None:
		return e.mean(dim = -1)
	return (e * frame_mask(e.shape[-1], olen)).sum(dim = -1) / (eps + f64(olen))


def weighted_mean_entropy(log_probs, olen = None, eps = 1e-9, eps_id = -1):
	"""sum_t e_t w_t / (eps + sum_t w_t), w_t = 1 - P(class eps_id at t) on valid frames, 0 beyond them"""
	lp = f64(log_probs)
	e = frame_entropy(lp)
	w = 1 - lp.exp()[:, eps_id]
	if olen is not None:
		w = w * frame_mask(e.shape[-1], olen)
	return (e * w).sum(dim = -1) / (eps + w.sum(dim = -1))


# ------------------------------------------------------------------------------------------------ argmax

def argmax(log_probs):
	"""torch.argmax over the class axis, restated: NaN ranks above every number; the lowest index among the maxima (among the NaNs, if there
	is one) wins; a row of all -inf gives 0.  (B, C, T) -> int64 (B, T)."""
	x = log_probs.detach().cpu().numpy()
	nan = np.isnan(x)
	with np.errstate(invalid = 'ignore'):
		top = np.where(nan, -np.inf, x).max(axis = 1, keepdims = True)
	first_max = np.argmax(x == top, axis = 1)  # (np.argmax of a bool array: the first True)
	first_nan = np.argmax(nan, axis = 1)
	return torch.from_numpy(np.where(nan.any(axis = 1), first_nan, first_max).astype(np.int64))


# ------------------------------------------------------------------------------------------------ row scaling, loss head

def scale_rows(grad, gscale = None, gdiv = None):
	"""grad[b] * gscale[b] / gdiv[b]; either factor may be absent"""
	g = f64(grad)
	s = torch.ones(g.shape[0], dtype = torch.float64)
	if gscale is not None:
		s = s * f64(gscale)
	if gdiv is not None:
		s = s / f64(gdiv)
	return g * s.view(-1, *[1] * (g.ndim - 1))


def loss_head(loss_vec, ylen, ent = None, accum = 1, metric_scale = 1.0, loss_scale = 1.0):
	"""The documented outputs of loss_head_kernel.  Returns (out3 float64, gvec fp32, skipped bool):
	  out3 = [mean(lv * w) / accum, mean(lv) * metric_scale, mean(ent) * metric_scale]   (ent None: 0)
	  gvec[b] = ((1 / accum) / B) * w[b] * loss_scale, evaluated in fp32 in exactly that order -- autograd's own; it is EXACT, not float64
	  skipped = the mean loss is not finite"""
	lv, w = f64(loss_vec), f64(ylen)
	B = lv.shape[0]
	cur = lv.mean()
	out3 = torch.stack([(lv * w).mean() / accum, cur * metric_scale, (f64(ent).mean() if ent is not None else torch.zeros((), dtype = torch.float64)) * metric_scale])
	one, acc, nb = (torch.tensor(v, dtype = torch.float32) for v in (1.0, float(accum), float(B)))
	gvec = ((one / acc) / nb) * ylen.detach().cpu().to(torch.float32) * torch.tensor(float(loss_scale), dtype = torch.float32)
	return out3, gvec, not bool(torch.isfinite(cur))


# ------------------------------------------------------------------------------------------------ lengths, instance norm

def output_lengths(xlen, B, T):
	"""ceil(frac * T) with the product taken in fp32, as the reference does ((lengths_fraction * T).ceil().long()); xlen None: T.  Exact."""
	if xlen is None:
		return torch.full((B, ), T, dtype = torch.int64)
	return (xlen.detach().cpu().to(torch.float32) * T).ceil().long()


def instnorm_stats(x, n = None):
	"""per-instance mean and BIASED variance over the first n[b] frames (n None: all), two-pass; (B, C) each"""
	x = f64(x)
	B, C, T = x.shape
	m = torch.ones(B, 1, T, dtype = torch.float64) if n is None else frame_mask(T, n).unsqueeze(1)
	cnt = m.sum(dim = -1)
	mean = (x * m).sum(dim = -1) / cnt
	var = (((x - mean.unsqueeze(-1)) * m) ** 2).sum(dim = -1) / cnt
	return mean, var


def instnorm(x, xlen, eps, T_out = None, fixed_mean = None, fixed_var = None):
	"""(x - mean) / sqrt(var + eps) on the valid frames t < n[b] = ceil(xlen[b] * T), zeros from frame n[b] up to T_out (an utterance with
	no valid frame is all zeros).  fixed_mean / fixed_var (C,): eval mode with running statistics instead of the instance's own."""
	xd = f64(x)
	B, C, T = xd.shape
	T_out = T if T_out is None else T_out
	n = output_lengths(xlen, B, T)
	if fixed_mean is not None:
		mean, var = f64(fixed_mean).view(1, C).expand(B, C), f64(fixed_var).view(1, C).expand(B, C)
	else:
		mean, var = instnorm_stats(xd, n)
	y = (xd - mean.unsqueeze(-1)) / torch.sqrt(var + eps).unsqueeze(-1)
	y = torch.where(frame_mask(T, n).unsqueeze(1).bool(), y, torch.zeros_like(y))  # (where, not a product: n = 0 has 0 / 0 statistics)
	return torch.cat([y, torch.zeros(B, C, T_out - T, dtype = torch.float64)], dim = -1)


def instnorm_running(x, running_mean, running_var, num_batches_tracked, momentum, eps, training, T_out = None):
	"""nn.InstanceNorm1d(track_running_stats = True): returns (y, running_mean, running_var, num_batches_tracked) after the call.
	training: y from the instance statistics; the running ones take, with weight `momentum`, the batch mean of the per-instance means and of
	the UNBIASED variances (T = 1: the biased one, there is nothing to unbias), and the counter counts the call (include/convasr_hip.h:
	torch's own InstanceNorm never counts, so the model passes no counter).  eval: y from the running statistics; nothing is written back."""
	xd = f64(x)
	T = xd.shape[-1]
	if not training:
		return instnorm(xd, None, eps, T_out, running_mean, running_var), f64(running_mean), f64(running_var), int(num_batches_tracked)
	mean, var = instnorm_stats(xd)
	unbiased = var * (T / (T - 1)) if T > 1 else var
	rm = (1 - momentum) * f64(running_mean) + momentum * mean.mean(dim = 0)
	rv = (1 - momentum) * f64(running_var) + momentum * unbiased.mean(dim = 0)
	return instnorm(xd, None, eps, T_out), rm, rv, int(num_batches_tracked) + 1


def normalize_signal(signal, eps = 1e-5, denom_multiplier = 1.0):
	"""x / ((max |x| + eps) * denom_multiplier) per row, of the float-converted signal (fp32 or int16 input)"""
	x = f64(signal)
	return x / ((x.abs().max(dim = -1, keepdim = True).values + eps) * denom_multiplier)


# ------------------------------------------------------------------------------------------------ exact ops

def convert_layout(x, dtype):
	"""a permutation of memory plus at most one rounding into `dtype`: the logical values are x.to(dtype)"""
	return x.detach().cpu().to(dtype)


def add16(a, b):
	"""the fp32 sum of two 16-bit values, rounded once into their type"""
	return (a.detach().cpu().float() + b.detach().cpu().float()).to(a.dtype)


def cast_scale(x, scale, dtype):
	"""(fp32(x) * scale) in fp32, then one rounding into `dtype` (none when dtype is fp32)"""
	return (x.detach().cpu().float() * torch.tensor(float(scale), dtype = torch.float32)).to(dtype)


def copy(src_bytes, nbytes):
	return src_bytes.detach().cpu()[:nbytes].clone()


def collate_pad(samples, rows, Tpad):
	"""samples: list of (rows, L_b) tensors of one dtype -> (B, rows, Tpad): the payload bit for bit, zeros behind it"""
	out = torch.zeros(len(samples), rows, Tpad, dtype = samples[0].dtype)
	for b, s in enumerate(samples):
		out[b, :, :s.shape[-1]] = s.reshape(rows, -1)
	return out
