"""The star-token Viterbi alignment without a GPU: the numpy restatement of convasr_star_alignment's rule (tests/_star_align_ref.py)
against a brute force over the subsets of the allowed gaps, the validity of the paths it returns, planted inputs, the plain alignment's
restatement under an all-false mask, and the wrapper's envelope and argument errors (every refusal precedes the first HIP call)."""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

import _ctc_align_ref as R
import _star_align_ref as A
import _star_ctc_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('convasr_star_alignment', 'convasr_star_alignment_parts', 'convasr_star_alignment_workspace_bytes', 'convasr_star_alignment_states_per_block', 'convasr_star_alignment_chunk_frames')


def ctc_viterbi(lp, labels, blank):
	"""Plain max-plus CTC Viterbi score in float64, written out state by state (independent of the arc table under test)."""
	T, S = lp.shape[0], len(labels)
	ext = [blank] * (2 * S + 1)
	ext[1::2] = labels
	L = len(ext)
	v = [-np.inf] * L
	v[0] = lp[0, blank]
	if L > 1:
		v[1] = lp[0, ext[1]]
	for t in range(1, T):
		w = [-np.inf] * L
		for s in range(L):
			best = v[s]
			if s >= 1:
				best = max(best, v[s - 1])
			if s >= 2 and s % 2 == 1 and ext[s] != ext[s - 2]:
				best = max(best, v[s - 2])
			w[s] = best + lp[t, ext[s]]
		v = w
	return max(v[L - 1], v[L - 2]) if L > 1 else v[0]


def brute_force(lp, labels, mask, blank, penalty, enter):
	"""max over the subsets A of the allowed gaps of |A| enter + the CTC Viterbi score of the labels with a star class at the gaps in A."""
	T, C = lp.shape
	wide = np.concatenate([lp, np.full((T, 1), penalty)], axis = 1)
	allowed = [g for g in range(len(labels) + 1) if mask[g]]
	best = -np.inf
	for k in range(len(allowed) + 1):
		for chosen in itertools.combinations(allowed, k):
			seq = []
			for g in range(len(labels) + 1):
				if g in chosen:
					seq.append(C)
				if g < len(labels):
					seq.append(int(labels[g]))
			best = max(best, k * enter + ctc_viterbi(wide, seq, blank))
	return best


def random_small_case(rng):
	T, S, C = rng.randint(1, 7), rng.randint(0, 4), 3  # two letters and the blank: repeats occur
	blank = int(rng.randint(0, C))
	labels = np.array([k for k in rng.randint(0, C - 1, size = S)], dtype = np.int64)
	labels[labels >= blank] += 1
	mask = rng.rand(S + 1) < rng.choice([0.0, 0.5, 1.0])
	lp = np.log(rng.dirichlet(np.ones(C), size = T))
	return lp, labels, mask, blank, -float(rng.exponential(1.0)), -float(rng.exponential(1.5))


def test_score_is_the_maximum_over_the_subsets_of_gaps_and_the_path_is_a_path():
	rng = np.random.RandomState(2024)
	infeasible, worst = 0, 0.0
	for case in range(600):
		lp, labels, mask, blank, penalty, enter = random_small_case(rng)
		got = A.align_one(lp, labels, mask, len(lp), blank, penalty, enter, dtype = np.float64)
		want = brute_force(lp, labels, mask, blank, penalty, enter)
		if not np.isfinite(want):
			infeasible += 1
			assert got.score == -np.inf and got.path is None and not got.alignment.any() and (got.star_begin == -1).all() and not got.star_frames.any(), case
			continue
		worst = max(worst, abs(got.score - want))
		assert abs(got.score - want) <= 1e-12, (case, got.score, want)
		# the path is a path of the lattice and its re-summed score is the score
		again = A.path_score(lp, labels, mask, got.path, blank, penalty, enter)
		assert again is not None and abs(again - got.score) <= 1e-12, (case, again, got.score)
		# star_begin / star_frames say exactly which frames it spends in which star; alignment the last frame in every label
		cls, gap, *_ = A.arcs(labels, mask, blank, enter, np.float64)
		label_of = np.cumsum((np.arange(len(cls)) % 2 == 1) & (cls != SR.STAR)) - 1
		for g in range(len(labels) + 1):
			frames = [t for t, s in enumerate(got.path) if s & 1 and gap[s] == g]
			assert got.star_frames[g] == len(frames) and got.star_begin[g] == (frames[0] if frames else -1), (case, g)
			assert frames == list(range(frames[0], frames[0] + len(frames))) if frames else True
		for j in range(len(labels)):
			frames = [t for t, s in enumerate(got.path) if s & 1 and cls[s] != SR.STAR and label_of[s] == j]
			assert frames and got.alignment[j] == frames[-1], (case, j)
	assert infeasible >= 30 and worst <= 1e-12, (infeasible, worst)


def test_the_arc_table_is_the_loss_lattice():
	"""The sum over paths through A.arcs' table equals _star_ctc_ref.lattice's likelihood: the two files hold one lattice."""
	rng = np.random.RandomState(7)
	for case in range(100):
		lp, labels, mask, blank, penalty, enter = random_small_case(rng)
		nll, _, _ = SR.lattice(lp, labels, mask, blank, penalty, enter)
		cls, gap, c, start, end = A.arcs(labels, mask, blank, enter, np.float64)
		em = lambda t: np.where(cls == SR.STAR, penalty, lp[t, np.where(cls == SR.STAR, 0, cls)])
		with np.errstate(invalid = 'ignore', divide = 'ignore'):
			a = start + em(0)
			for t in range(1, len(lp)):
				a = SR._lse(np.stack([SR._shift(a, d) + c[d] for d in range(5)])) + em(t)
			total = SR._lse((a + end)[:, None])[0]
		assert (np.isinf(nll) and np.isinf(total)) or abs(-total - nll) <= 1e-9, (case, total, nll)


def test_float32_restatement_rounds_once_per_step():
	"""The float32 run keeps float32 throughout (align_one asserts the dtype every frame) and stays within rounding of the float64 one."""
	rng = np.random.RandomState(5)
	for case in range(50):
		lp, labels, mask, blank, penalty, enter = random_small_case(rng)
		lo, hi = A.align_one(lp.astype(np.float32), labels, mask, len(lp), blank, penalty, enter), A.align_one(lp, labels, mask, len(lp), blank, penalty, enter, dtype = np.float64)
		assert lo.score.dtype == np.float32
		assert np.isinf(hi.score) == np.isinf(lo.score) and (np.isinf(hi.score) or abs(float(lo.score) - hi.score) <= 1e-5 * (1 + abs(hi.score)))


C = 38


def test_planted_inputs_return_their_planted_positions():
	for seed, S, inserts, allowed in ((1, 40, {17: 60}, 'all'), (2, 25, {0: 30, 25: 45}, 'all'), (3, 30, {10: 20, 11: 35}, 'inserts'), (4, 12, {}, 'all'), (5, 1, {1: 9}, 'all')):
		labels = A.random_labels(seed, S, C, C - 1)
		T = 3 * S + sum(inserts.values()) + 20
		lp, pos, runs = A.planted(seed, T, labels, C, C - 1, inserts, input_length = T - 5)
		mask = np.ones(S + 1, dtype = bool) if allowed == 'all' else np.array([g in inserts for g in range(S + 1)])
		got = A.align_one(lp, labels, mask, T - 5, C - 1, -1.0, -2.0)
		assert np.array_equal(got.alignment, pos), (seed, got.alignment, pos)
		for g in range(S + 1):
			assert (got.star_begin[g], got.star_frames[g]) == (runs[g] if g in runs else (-1, 0)), (seed, g)


def test_all_false_mask_is_the_plain_alignment_on_planted_inputs():
	for seed, T, S, Tb in ((1, 200, 60, 200), (2, 513, 130, 500), (3, 40, 1, 17)):
		lp, targets, pos = R.planted(seed, T, S, C, C - 1, 12.0, input_length = Tb)
		got = A.align_one(lp, targets, np.zeros(S + 1, dtype = bool), Tb, C - 1, -1.0, -2.0)
		assert np.array_equal(got.alignment, R.alignment_one(lp, targets, Tb, S, blank = C - 1)) and np.array_equal(got.alignment, pos)
		assert not got.star_frames.any() and (got.star_begin == -1).all()


def test_star_pieces_on_hand_written_outputs():
	from convasr_amd import ctc
	result = types.SimpleNamespace(
		alignment = torch.tensor([[2, 4, 30, 33, 36, 0], [1, 3, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0]]),
		star_begin = torch.tensor([[-1, -1, 6, -1, 34, -1, -1], [0, -1, 5, -1, -1, -1, -1], [-1] * 7, [0, 7, -1, -1, -1, -1, -1]]),
		star_frames = torch.tensor([[0, 0, 20, 0, 1, 0, 0], [1, 0, 10, 0, 0, 0, 0], [0] * 7, [4, 3, 0, 0, 0, 0, 0]]),
		score = torch.tensor([-3.0, -2.0, float('-inf'), -1.0]), input_lengths = torch.tensor([40, 15, 9, 10]))
	targets, ylen = torch.zeros(4, 6, dtype = torch.int64), torch.tensor([5, 2, 3, 1])
	every = ctc.star_pieces(result, targets, ylen, 1)
	assert every[0].stars == [(2, 6, 25), (4, 34, 34)] and every[0].pieces == [(0, 2, 0, 5), (2, 2, 26, 33), (4, 1, 35, 39)]
	assert every[1].stars == [(0, 0, 0), (2, 5, 14)] and every[1].pieces == [(0, 2, 1, 4)]
	assert every[2].stars == [] and every[2].pieces == []  # no path
	assert every[3].stars == [(0, 0, 3), (1, 7, 9)] and every[3].pieces == [(0, 1, 4, 6)]
	long = ctc.star_pieces(result, targets, ylen, 4)  # short stars stay inside their pieces
	assert long[0].stars == [(2, 6, 25)] and long[0].pieces == [(0, 2, 0, 5), (2, 3, 26, 39)]
	assert long[1].stars == [(2, 5, 14)] and long[1].pieces == [(0, 2, 0, 4)]
	assert long[3].stars == [(0, 0, 3)] and long[3].pieces == [(0, 1, 4, 9)]


def test_unit_table_of_the_wrapper():
	from convasr_amd import ops
	targets = torch.tensor([[5, 7, 7, 99], [3, 0, 0, 0], [1, 2, 3, 4]])
	ylen = torch.tensor([3, 1, 0])
	mask = torch.tensor([[True, False, True, True, True], [False, True, True, True, True], [True, True, False, False, False]])
	units, n = ops.star_alignment_units(targets, ylen, mask, 38)
	assert units.dtype == torch.int32 and n.dtype == torch.int32 and units.shape == (3, 9)
	assert n.tolist() == [6, 2, 1]
	assert units[0, :6].tolist() == [-2, 5, 7, -4, 7, -5] and units[1, :2].tolist() == [3, -3] and units[2, :1].tolist() == [-2]
	for b, S in enumerate(ylen.tolist()):  # the same units as the loss's restatement lists
		ucls, ugap = SR.units_of(targets[b, :S].numpy(), mask[b, :S + 1].numpy())
		assert [(-(g + 2) if c == SR.STAR else c) for c, g in zip(ucls, ugap)] == units[b, :n[b]].tolist()
	assert ops.star_alignment_units(torch.tensor([[40, -1]]), torch.tensor([2]), torch.zeros(1, 3, dtype = torch.bool), 38)[0][0, :2].tolist() == [-1, -1]


def test_wiring_envelope_and_argument_errors_without_a_gpu():
	from convasr_amd import _lib, ctc, ops
	header = open(os.path.join(ROOT, 'include', 'convasr_hip.h')).read()
	lib = _lib.load()
	for name in NEW:
		assert re.search(r'\b' + name + r'\s*\(', header), name
		assert name in _lib._SIGNATURES and hasattr(lib, name), name
	assert 'log-sum-exp' in header[header.index('BEST PATH through the star lattice'):header.index('int convasr_star_alignment_states_per_block')]
	sb, ch = ops.star_alignment_tiles()
	assert (sb, ch) == (lib.convasr_star_alignment_states_per_block(), lib.convasr_star_alignment_chunk_frames()) and sb % 2 == 0 and 16 <= ch <= 4096
	assert ops.STAR_ALIGN_WORKSPACE_CAP == 16 << 30
	assert callable(ctc.star_alignment) and callable(ctc.star_alignment_bct) and callable(ctc.StarCTC.align) and callable(ctc.star_pieces)
	most = 2 * 131071 + 1
	assert lib.convasr_star_alignment_workspace_bytes(1, 1 << 20, 10) > 0 and lib.convasr_star_alignment_workspace_bytes(65535, 4, most) > 0
	for shape in ((1, (1 << 20) + 1, 10), (65536, 4, 10), (1, 4, most + 1), (0, 4, 10), (1, 0, 10), (1, 4, 0)):
		assert lib.convasr_star_alignment_workspace_bytes(*shape) == -1, shape
	# an hour at 48,000 labels with 9,000 stars fits the cap
	assert lib.convasr_star_alignment_workspace_bytes(1, 180000, 57000) < ops.STAR_ALIGN_WORKSPACE_CAP
	# the C entry refuses before any HIP call (the pointers are never read)
	buf = ctypes.create_string_buffer(64)
	one = ctypes.cast(buf, ctypes.c_void_p)
	def entry(B = 1, T = 50, C = 38, S_max = 20, N_max = 41, blank = 37, chunk = 0, parts = 3, pen = -1.0, ent = -2.0, nbytes = 1 << 40):
		return lib.convasr_star_alignment_parts(one, one, one, one, one, pen, ent, one, one, one, one, one, nbytes, B, T, C, S_max, N_max, blank, chunk, parts, None)
	einval, eunsupported = -1, -3
	for kw, code in ((dict(pen = 0.5), einval), (dict(ent = 1e-3), einval), (dict(pen = float('-inf')), einval), (dict(chunk = 8), einval), (dict(chunk = 4097), einval), (dict(parts = 0), einval),
	                 (dict(parts = 4), einval), (dict(blank = 38), einval), (dict(nbytes = 1 << 20, T = 100000, N_max = 400, S_max = 200), einval), (dict(S_max = 131072, N_max = most), eunsupported),
	                 (dict(N_max = most + 1, S_max = 131071), eunsupported), (dict(T = (1 << 20) + 1), eunsupported), (dict(B = 65536), eunsupported)):
		assert entry(**kw) == code, (kw, lib.convasr_last_error())
	# the Python wrapper: arguments first (no device needed), then the device
	lp, tg, il, tl = torch.zeros(1, 50, 38), torch.zeros(1, 20, dtype = torch.int64), torch.tensor([50]), torch.tensor([20])
	mask = torch.ones(1, 21, dtype = torch.bool)
	good = dict(log_probs_btc = lp, targets = tg, input_lengths = il, target_lengths = tl, blank = 37, star_mask = mask, star_penalty = -1.0, star_enter = -2.0)
	for kw in (dict(star_penalty = 0.1), dict(star_enter = 1), dict(star_penalty = float('-inf')), dict(star_enter = None), dict(star_mask = mask[:, :20]), dict(star_mask = mask.to(torch.uint8)),
	           dict(chunk_frames = 8), dict(chunk_frames = 5000), dict(blank = 38), dict(target_lengths = torch.tensor([20, 20])), dict(log_probs_btc = lp[0])):
		with pytest.raises(ValueError):
			ops.star_ctc_alignment(**dict(good, **kw))
	for kw in (dict(targets = torch.zeros(1, 131072, dtype = torch.int64), star_mask = torch.zeros(1, 131073, dtype = torch.bool)), dict(log_probs_btc = torch.zeros(1, (1 << 20) + 1, 2), blank = 1)):
		with pytest.raises(_lib.ConvasrHipError, match = 'outside the envelope'):
			ops.star_ctc_alignment(**dict(good, **kw))
	with pytest.raises(ValueError):
		ctc.StarCTC('all', penalty = 0.5, enter = -1.0)
