"""Float64 numpy restatement of the N-best MWER rule (include/convasr_hip.h: convasr_mwer_loss has it).  The CTC lattice of a
hypothesis is tests/_star_ctc_ref.py's with no star anywhere, which is the plain lattice.  Shared by tests/test_mwer_ref.py (which pins it
against F.ctc_loss, a brute force over every frame labelling and float64 autograd) and tests/test_mwer_gpu.py (which pins the kernels
against it)."""
import numpy as np

from _star_ctc_ref import lattice


def weights(ll, risk, scale):
	"""One utterance: ll (N,) with -inf for a hypothesis that does not take part -> (loss, p (N,), w (N,), E, rbar)."""
	N = len(ll)
	part = np.isfinite(ll)
	p, w = np.zeros(N), np.zeros(N)
	if not part.any():
		return 0.0, p, w, 0.0, 0.0
	z = scale * (ll[part] - ll[part].max())
	e = np.exp(z)
	p[part] = e / e.sum()
	E = float((p[part] * risk[part]).sum())
	rbar = float(risk[part].mean())
	if part.sum() < 2:
		return 0.0, p, w, E, rbar
	w[part] = scale * p[part] * (risk[part] - E)
	return E - rbar, p, w, E, rbar


def mwer_ref(log_probs, hyps, hyp_lengths, olen, risk, blank, scale):
	"""log_probs (B, C, T), hyps (B, N, L_max), hyp_lengths (B, N), olen (B,), risk (B, N): array-likes.  Returns float64 (loss (B,), grad
	(B, C, T), hyp_nll (B, N), hyp_posterior (B, N), w (B, N))."""
	lp = np.asarray(log_probs, dtype = np.float64)
	hyps, hyp_lengths, olen, risk = np.asarray(hyps), np.asarray(hyp_lengths), np.asarray(olen), np.asarray(risk, dtype = np.float64)
	B, C, T = lp.shape
	N = hyp_lengths.shape[1]
	hyps = hyps.reshape(B, N, -1)
	L_max = hyps.shape[2]
	loss, grad, nll, post, wts = np.zeros(B), np.zeros((B, C, T)), np.full((B, N), np.inf), np.zeros((B, N)), np.zeros((B, N))
	for b in range(B):
		Tb = int(olen[b])
		occ = [None] * N
		if 1 <= Tb <= T:
			rows = lp[b, :, :Tb].T
			for n in range(N):
				L = int(hyp_lengths[b, n])
				if 0 <= L <= L_max:
					nll[b, n], occ[n], _ = lattice(rows, hyps[b, n, :L], np.zeros(L + 1, dtype = bool), blank, 0.0, 0.0)
		loss[b], post[b], wts[b], _, _ = weights(-nll[b], risk[b], scale)
		for n in range(N):
			if wts[b, n] != 0.0:
				grad[b, :, :Tb] += wts[b, n] * occ[n].T
	return loss, grad, nll, post, wts
