"""float64 restatement of the batch-norm / residual / activation family (convasr_amd/csrc/bn.hip), plain torch on the CPU.

Layout here is rows-major (B, T, C): the memory order of the kernels' channels-last tensors.  Every argument is converted to float64
first; per-channel vectors are (C,).  The backward takes dz/dpre from autograd on the forward expression, not from the kernels'
formulas; the closed forms that follow it (sums, dy, the coefficient triple) are the textbook batch-norm backward and are themselves
checked against autograd through F.batch_norm in tests/test_bn_ref.py."""
import torch
import torch.nn.functional as F

from oracle import convasr_oracle as O

NONLINS = dict(none = None, relu = ('relu', ), hardtanh = ('hardtanh', 0, 20), leaky_relu = ('leaky_relu', 0.01))


def f64(t):
	return None if t is None else t.detach().to(device = 'cpu', dtype = torch.float64)


def activation(pre, nonlin):
	return pre if nonlin is None else O.activation(pre, nonlin)


def bounds(nonlin):
	"""pre-activation values at which the gradient gate switches"""
	return () if nonlin is None else ((0.0, 20.0) if nonlin[0] == 'hardtanh' else (0.0, ))


def frame_mask(B, T, xlen):
	"""(B, T, 1) float64, 1 on valid frames: ceil(xlen * T) evaluated in fp32 like the reference (models.py:614)"""
	lengths = O.compute_output_lengths(T, None if xlen is None else xlen.detach().cpu().float(), B)
	return O.temporal_mask(T, lengths).to(torch.float64).unsqueeze(-1)


def pre_activation(y, scale, shift, res = (), rscale = (), rshift = ()):
	pre = f64(y) if scale is None else f64(y) * f64(scale) + f64(shift)
	for r, t in enumerate(res):
		sc = rscale[r] if r < len(rscale) else None
		pre = pre + (f64(t) if sc is None else f64(t) * f64(sc) + f64(rshift[r]))
	return pre


def pre_magnitude(y, scale, shift, res = (), rscale = (), rshift = ()):
	"""sum of the magnitudes of the addends of the pre-activation: the scale of its fp32 rounding error"""
	mag = f64(y).abs() if scale is None else (f64(y) * f64(scale)).abs() + f64(shift).abs()
	for r, t in enumerate(res):
		sc = rscale[r] if r < len(rscale) else None
		mag = mag + (f64(t).abs() if sc is None else (f64(t) * f64(sc)).abs() + f64(rshift[r]).abs())
	return mag


def near_bound(y, scale, shift, res, rscale, rshift, nonlin, rel = 1e-5):
	"""bool (B, T, C): float64 pre-activation within rel * (magnitude of the addends) of a gate boundary"""
	pre, mag = pre_activation(y, scale, shift, res, rscale, rshift), pre_magnitude(y, scale, shift, res, rscale, rshift)
	near = torch.zeros_like(pre, dtype = torch.bool)
	for bound in bounds(nonlin):
		near |= (pre - bound).abs() <= rel * mag  # (<=: an exact tie of addends that are all zero counts)
	return near


def forward(y, scale, shift, res, rscale, rshift, nonlin, keep, xlen):
	"""z = mask * keep * act(y * scale + shift + sum_r (res_r * rscale_r + rshift_r)); keep: None or a tensor of 0 / keep_scale values.
	Returns (z, pre)."""
	B, T, _ = y.shape
	pre = pre_activation(y, scale, shift, res, rscale, rshift)
	z = activation(pre, nonlin) * frame_mask(B, T, xlen)
	return (z if keep is None else z * f64(keep)), pre


def grad_pre(pre, nonlin, keep, xlen, dz):
	"""g = dz * dz/dpre by autograd on the forward expression; also the gate bits (the gradient passes: dz/dpre != 0)"""
	B, T, _ = pre.shape
	p = pre.detach().clone().requires_grad_(True)
	z = activation(p, nonlin) * frame_mask(B, T, xlen)
	if keep is not None:
		z = z * f64(keep)
	(g, ) = torch.autograd.grad(z, p, f64(dz))
	(unit, ) = torch.autograd.grad(activation(p, nonlin) * frame_mask(B, T, xlen) * (1.0 if keep is None else f64(keep)), p, torch.ones_like(p))
	return g, unit != 0


def bn_sums(g, y, mean, invstd):
	"""(sum g, sum g * xhat) per channel, xhat = (y - mean) * invstd"""
	xhat = (f64(y) - f64(mean)) * f64(invstd)
	return g.sum(dim = (0, 1)), (g * xhat).sum(dim = (0, 1))


def bn_coef(sg, sgx, n, gamma, mean, invstd):
	"""(A, B, D) with dy = A * g + B * y + D"""
	gm = torch.ones_like(sg) if gamma is None else f64(gamma)
	m, istd = f64(mean), f64(invstd)
	msg, msgx = sg / n, sgx / n
	return gm * istd, -gm * istd * istd * msgx, gm * istd * (m * istd * msgx - msg)


def bn_dy(g, y, gamma, mean, invstd, sg = None, sgx = None):
	"""dy = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)); the sums default to those of g itself"""
	n = g.shape[0] * g.shape[1]
	if sg is None:
		sg, sgx = bn_sums(g, y, mean, invstd)
	gm = 1.0 if gamma is None else f64(gamma)
	xhat = (f64(y) - f64(mean)) * f64(invstd)
	return gm * f64(invstd) * (g - f64(sg) / n - xhat * f64(sgx) / n)


def finalize(s1, s2, n, gamma, beta, running_mean, running_var, momentum, eps):
	"""Training-mode batch-norm statistics from per-channel sum and sum of squares over n elements: dict of mean, var (biased, clamped
	at 0), invstd, scale, shift and the updated running statistics (unbiased variance estimate; n = 1: the biased one)."""
	m = f64(s1) / n
	var = (f64(s2) / n - m * m).clamp_min(0.0)
	invstd = 1.0 / torch.sqrt(var + eps)
	gm = torch.ones_like(m) if gamma is None else f64(gamma)
	bt = torch.zeros_like(m) if beta is None else f64(beta)
	out = dict(mean = m, var = var, invstd = invstd, scale = gm * invstd, shift = bt - m * gm * invstd)
	if running_mean is not None:
		out['running_mean'] = (1 - momentum) * f64(running_mean) + momentum * m
		out['running_var'] = (1 - momentum) * f64(running_var) + momentum * (var * n / (n - 1) if n > 1 else var)
	return out


def eval_scale_shift(gamma, beta, running_mean, running_var, eps):
	invstd = 1.0 / torch.sqrt(f64(running_var) + eps)
	gm = torch.ones_like(invstd) if gamma is None else f64(gamma)
	bt = torch.zeros_like(invstd) if beta is None else f64(beta)
	return gm * invstd, bt - f64(running_mean) * gm * invstd
