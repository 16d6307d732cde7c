"""convasr_nw_align_long and convasr_edit_distance_long on the GPU, exactly (== / torch.equal, no tolerance anywhere): against the Python
restatements tests/_align_ref.nw_align and tests/_metrics_ref.levenshtein, against the one-wave kernels ops.nw_align / ops.edit_distance
wherever both take the arguments, and through metrics.cer_wer / align_strings / token_cer_wer past the 16,383 units those stopped at."""
import random

import numpy as np
import pytest
import torch

import _align_ref as A
import _metrics_ref as R
from _align_golden import ref_aligner

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SCORE_SETS = [A.WORD_SCORES, A.CHAR_SCORES, (1, -1, -1, -1), (0, 0, 0, 0), (3, 1, -2, -5), (2048, -2048, -2048, -2048)]


def tile():
	from convasr_amd import ops
	return ops.nw_align_long_tile()


def pack(pairs, pad_a = 0, pad_b = 0, poison = None):
	"""(a, b) id lists -> int32 device tensors (N, La + pad_a), (N, Lb + pad_b) and the lengths; poison: the id past every length."""
	N = len(pairs)
	La, Lb = max(len(a) for a, b in pairs) + pad_a, max(len(b) for a, b in pairs) + pad_b
	ta, tb = np.full((N, La), poison or 0, dtype = np.int32), np.full((N, Lb), poison or 0, dtype = np.int32)
	for p, (a, b) in enumerate(pairs):
		ta[p, :len(a)], tb[p, :len(b)] = a, b
	al, bl = torch.tensor([len(a) for a, b in pairs], dtype = torch.int32), torch.tensor([len(b) for a, b in pairs], dtype = torch.int32)
	return torch.from_numpy(ta).to(DEV), al.to(DEV), torch.from_numpy(tb).to(DEV), bl.to(DEV)


def rows(result, N):
	"""The four tensors of an alignment call -> per pair (a_index, b_index, score) cut at n_cols; checks dtypes and the -1 fill."""
	ai, bi, n, score = [t.cpu() for t in result]
	assert ai.shape == bi.shape and ai.shape[0] == N and ai.dtype == bi.dtype == n.dtype == score.dtype == torch.int32
	cols = torch.arange(ai.shape[1])[None, :] >= n[:, None]
	assert bool((ai[cols] == -1).all()) and bool((bi[cols] == -1).all())
	ai, bi, n, score = ai.numpy(), bi.numpy(), n.tolist(), score.tolist()
	return [(ai[p, :n[p]].tolist(), bi[p, :n[p]].tolist(), score[p]) for p in range(N)]


def check_align(pairs, scores, against_short = True, **kwargs):
	from convasr_amd import ops
	t = pack(pairs)
	got = ops.nw_align_long(*t, scores, **kwargs)
	assert got[0].shape == (len(pairs), t[0].shape[1] + t[2].shape[1])
	if against_short:
		for x, y in zip(got, ops.nw_align(*t, scores)):
			assert torch.equal(x, y)
	for (a, b), g in zip(pairs, rows(got, len(pairs))):
		assert g == A.nw_align(a, b, scores), (len(a), len(b), scores)
	return got


def check_distance(pairs, against_short = True, **kwargs):
	from convasr_amd import _lib, ops
	t = pack(pairs)
	got = ops.edit_distance_long(*t, **kwargs)
	assert got.shape == (len(pairs),) and got.dtype == torch.int32
	if against_short:
		short, _ = ops.edit_distance(t[0].long(), t[1].long(), t[2].long(), t[3].long(), _lib.METRIC_CHARS, -1)
		assert torch.equal(got, short)
	assert got.cpu().tolist() == [R.levenshtein(a, b) for a, b in pairs]
	return got


def seq(rng, n, alpha):
	return [rng.randrange(alpha) for _ in range(n)]


def noisy_copy(rng, a, alpha, p = 0.05):
	out = []
	for x in a:
		r = rng.random()
		if r < p / 3:
			continue
		out.append(rng.randrange(alpha) if r < 2 * p / 3 else x)
		if r > 1 - p / 3:
			out.append(rng.randrange(alpha))
	return out


def edge_pairs(alpha):
	"""Every (la, lb) around the chunk and the tile edges; b is a noisy copy of a where the lengths allow it, so paths cross tile corners."""
	T = tile()
	edges = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
	rng = random.Random(1000 + alpha)
	pairs = []
	for n, la in enumerate(edges):
		for m, lb in enumerate(edges):
			a = seq(rng, la, alpha)
			pairs.append((a, (noisy_copy(rng, a, alpha) + seq(rng, lb, alpha))[:lb] if (n + m) % 2 else seq(rng, lb, alpha)))
	return pairs


@pytest.mark.parametrize('scores', SCORE_SETS, ids = lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('alpha', [2, 38])
def test_edges_in_one_batched_call(alpha, scores):
	check_align(edge_pairs(alpha), scores)


@pytest.mark.parametrize('alpha', [2, 38])
def test_distance_edges_in_one_batched_call(alpha):
	check_distance(edge_pairs(alpha))


def test_several_tiles_in_both_directions():
	T = tile()
	rng = random.Random(21)
	la, lb = 3 * T + 17, 5 * T + 3
	a = seq(rng, la, 38)
	long_b = (noisy_copy(rng, a, 38) + seq(rng, lb, 38))[:lb]
	b = seq(rng, lb, 38)
	pairs = [(a, long_b), (long_b, a), (noisy_copy(rng, b, 38)[:la], b), (seq(rng, la, 2), seq(rng, lb, 2)), (seq(rng, lb, 2), seq(rng, la, 2)),
	         (b[2 * T - 5:2 * T + 40], b), (b, b[T + 3:T + 300]), (a, a)]
	check_align(pairs, A.CHAR_SCORES)
	check_align(pairs[:5], (3, 1, -2, -5))
	check_distance(pairs)


def test_buffers_wider_than_the_lengths():
	from convasr_amd import ops
	T = tile()
	rng = random.Random(22)
	pairs = [(seq(rng, la, 3), seq(rng, lb, 3)) for la, lb in [(T + 5, 2 * T - 1), (0, 9), (64, T), (2 * T, 3), (T, T)]]
	want = [A.nw_align(a, b, A.CHAR_SCORES) for a, b in pairs]
	a, al, b, bl = pack(pairs, pad_a = T + 9, pad_b = 70, poison = 1)  # id 1 is in the alphabet: a unit read past a length would change a score
	assert rows(ops.nw_align_long(a, al, b, bl, A.CHAR_SCORES), len(pairs)) == want
	assert ops.edit_distance_long(a, al, b, bl).cpu().tolist() == [R.levenshtein(x, y) for x, y in pairs]
	# lengths above the buffer and below zero are clamped to [0, La] / [0, Lb]
	a, _, b, _ = pack(pairs)
	al, bl = torch.tensor([10 ** 6, -3, 2 * T, 2 ** 31 - 1, 7], dtype = torch.int32, device = DEV), torch.tensor([-1, 5, 10 ** 9, 2, -2 ** 31], dtype = torch.int32, device = DEV)
	La, Lb = a.shape[1], b.shape[1]
	clamped = [(a[p, :min(max(int(al[p]), 0), La)].tolist(), b[p, :min(max(int(bl[p]), 0), Lb)].tolist()) for p in range(len(pairs))]
	assert rows(ops.nw_align_long(a, al, b, bl, A.CHAR_SCORES), len(pairs)) == [A.nw_align(x, y, A.CHAR_SCORES) for x, y in clamped]
	assert ops.edit_distance_long(a, al, b, bl).cpu().tolist() == [R.levenshtein(x, y) for x, y in clamped]


def test_two_runs_give_identical_bits():
	"""Nothing depends on what the workspace held: the allocator's blocks are dirtied between the runs."""
	from convasr_amd import ops
	T = tile()
	N, L = 12, 2 * T + 40
	g = torch.Generator().manual_seed(23)
	a, b = torch.randint(0, 3, (N, L), dtype = torch.int32, generator = g).to(DEV), torch.randint(0, 3, (N, L + 30), dtype = torch.int32, generator = g).to(DEV)
	al, bl = torch.randint(0, L + 1, (N,), generator = g).to(DEV), torch.randint(0, L + 31, (N,), generator = g).to(DEV)
	first, first_d = ops.nw_align_long(a, al, b, bl, A.CHAR_SCORES), ops.edit_distance_long(a, al, b, bl)
	torch.empty(1 << 26, dtype = torch.uint8, device = DEV).fill_(0xA5)  # (dirty the allocator's blocks between the runs)
	second, second_d = ops.nw_align_long(a, al, b, bl, A.CHAR_SCORES), ops.edit_distance_long(a, al, b, bl)
	assert all(torch.equal(x, y) for x, y in zip(first, second)) and torch.equal(first_d, second_d)


def test_more_pairs_than_one_grid_dimension_holds():
	"""A launch carries 32,768 pairs in grid.y and the rest in grid.z: pairs on both sides of that edge, and a last grid.z slice that is
	not full."""
	from convasr_amd import _lib, ops
	N, L = 2 * 32768 + 5, 3
	g = torch.Generator().manual_seed(30)
	a, b = torch.randint(0, 2, (N, L), dtype = torch.int32, generator = g).to(DEV), torch.randint(0, 2, (N, L + 1), dtype = torch.int32, generator = g).to(DEV)
	al, bl = torch.randint(0, L + 1, (N,), dtype = torch.int32, generator = g).to(DEV), torch.randint(0, L + 2, (N,), dtype = torch.int32, generator = g).to(DEV)
	got = ops.nw_align_long(a, al, b, bl, A.CHAR_SCORES)
	assert all(torch.equal(x, y) for x, y in zip(got, ops.nw_align(a, al, b, bl, A.CHAR_SCORES)))
	dist = ops.edit_distance_long(a, al, b, bl)
	assert torch.equal(dist, ops.edit_distance(a.long(), al.long(), b.long(), bl.long(), _lib.METRIC_CHARS, -1)[0])
	picked = [0, 1, 32767, 32768, 32769, 65535, 65536, N - 1]
	per_pair = rows([t[picked] for t in got], len(picked))
	for p, r in zip(picked, per_pair):
		x, y = a[p, :int(al[p])].tolist(), b[p, :int(bl[p])].tolist()
		assert r == A.nw_align(x, y, A.CHAR_SCORES) and int(dist[p]) == R.levenshtein(x, y), p


def test_just_past_the_old_envelope():
	rng = random.Random(24)
	a = seq(rng, 16500, 38)
	b = (noisy_copy(rng, a, 38) + seq(rng, 400, 38))[:16400]
	assert len(b) == 16400
	check_align([(a, b)], A.CHAR_SCORES, against_short = False)
	check_distance([(a, b)], against_short = False)


def test_planted_alignment_near_the_limit():
	"""100,000 distinct ids against a copy with isolated edits of fresh ids: with distinct ids and the CHAR scores the planted alignment is
	the only optimal one, so the expected rows, score and distance come from the edit list, not from a reference run."""
	from convasr_amd import ops
	n = 100_000
	rng = random.Random(25)
	spots = sorted(rng.sample(range(50, n - 50, 40), 600))  # isolated: 40 units apart at least, none near an end
	kinds = {s: rng.choice('sdi') for s in spots}
	a = list(range(n))
	b, ai, bi, fresh = [], [], [], n
	match, sub, dele, ins = A.CHAR_SCORES
	score = 0
	for i in range(n):
		kind = kinds.get(i)
		if kind == 'd':  # a[i] has no partner
			ai.append(i); bi.append(-1)
			score += dele
			continue
		if kind == 'i':  # a fresh unit of b before a[i]
			ai.append(-1); bi.append(len(b))
			b.append(fresh)
			fresh += 1
			score += ins
		ai.append(i); bi.append(len(b))
		b.append(fresh if kind == 's' else i)
		fresh += kind == 's'
		score += sub if kind == 's' else match
	ta, al, tb, bl = pack([(a, b)])
	got_a, got_b, cols, got_score = ops.nw_align_long(ta, al, tb, bl, A.CHAR_SCORES)
	assert int(cols[0]) == len(ai) and int(got_score[0]) == score
	assert torch.equal(got_a[0, :len(ai)].cpu(), torch.tensor(ai, dtype = torch.int32)) and torch.equal(got_b[0, :len(bi)].cpu(), torch.tensor(bi, dtype = torch.int32))
	assert bool((got_a[0, len(ai):] == -1).all()) and bool((got_b[0, len(bi):] == -1).all())
	assert ops.edit_distance_long(ta, al, tb, bl).cpu().tolist() == [len(spots)]
	assert ops.edit_distance_long(tb, bl, ta, al).cpu().tolist() == [len(spots)]


def _text(rng, n_chars):
	"""About n_chars characters of lowercase words."""
	words, total = [], 0
	while total < n_chars:
		words.append(''.join(rng.choice('abcdefghij') for _ in range(rng.randrange(1, 9))))
		total += len(words[-1]) + 1
	return words


def _edited(rng, words, p = 0.05):
	out = []
	for w in words:
		r = rng.random()
		if r < p / 3:
			continue
		out.append(w[::-1] + 'k' if r < 2 * p / 3 else w)
		if r > 1 - p / 3:
			out.append('zz')
	return out


def test_cer_wer_routes_only_the_long_pair_to_the_long_kernel():
	from convasr_amd import metrics, ops
	rng = random.Random(26)
	ref_words = _text(rng, 22000)
	refs = ['a b c', 'hello world', ' '.join(ref_words), '', 'same same']
	hyps = ['a c', 'helo  wrld x', ' '.join(_edited(rng, ref_words)), 'x', 'same same']
	assert len(refs[2].replace(' ', '')) > 17000 and len(ref_words) < 16383
	launches, real = [], ops.call
	ops.call = lambda name, *args: (launches.append(name), real(name, *args))[1]
	try:
		cers, wers = metrics.cer_wer(hyps, refs)
	finally:
		ops.call = real
	assert launches == ['convasr_edit_distance', 'convasr_edit_distance_long', 'convasr_edit_distance']  # characters: short pairs, the long pair; words: all short
	assert cers == [R.cer(h, r) for h, r in zip(hyps, refs)] and wers == [R.wer(h, r) for h, r in zip(hyps, refs)]
	assert metrics.cer_wer(hyps[:2], refs[:2], route = 'long') == (cers[:2], wers[:2])
	assert metrics.cer(hyp = hyps[2], ref = refs[2]) == cers[2]


def test_align_strings_on_17000_words():
	from convasr_amd import metrics
	rng = random.Random(27)
	vocab = [''.join(rng.choice('abcdefghij') for _ in range(rng.randrange(2, 7))) for _ in range(400)]
	ref_words = [rng.choice(vocab) for _ in range(17000)]
	hyp, ref = ' '.join(_edited(rng, ref_words)), ' '.join(ref_words)
	assert metrics.align_strings(hyp = hyp, ref = ref) == metrics.align_strings(hyp = hyp, ref = ref, aligner = ref_aligner)


def test_token_cer_wer_on_20000_tokens():
	from convasr_amd import metrics
	g = torch.Generator().manual_seed(28)
	B, L, space = 2, 20000, 1
	ref = torch.randint(2, 30, (B, L), generator = g)
	ref[torch.rand(B, L, generator = g) < 0.18] = space
	hyp = ref.clone()
	edit = torch.rand(B, L, generator = g) < 0.05
	hyp[edit] = torch.randint(1, 30, (int(edit.sum()),), generator = g)
	hlen, rlen = torch.tensor([L, L - 700]), torch.tensor([L - 3, L])
	c, w = metrics.token_cer_wer(hyp.to(DEV), hlen.to(DEV), ref.to(DEV), rlen.to(DEV), space)
	assert c.dtype == w.dtype == torch.float64 and c.shape == w.shape == (B,) and c.is_cuda
	for b in range(B):
		h, r = hyp[b, :hlen[b]].tolist(), ref[b, :rlen[b]].tolist()
		for got, mode in ((c, 0), (w, 1)):
			d, n = R.edit_distance(h, r, mode, space)
			assert float(got[b]) == d / max(n, 1), (b, mode)
	# (B, K, L) hypotheses, the long route forced on a short batch: the same numbers as the short route
	hyp3 = torch.stack([hyp[:, :300], ref[:, :300]], dim = 1).to(DEV)
	len3 = torch.tensor([[300, 250], [0, 300]]).to(DEV)
	short = metrics.token_cer_wer(hyp3, len3, ref[:, :300].to(DEV), torch.tensor([300, 280]).to(DEV), space)
	forced = metrics.token_cer_wer(hyp3, len3, ref[:, :300].to(DEV), torch.tensor([300, 280]).to(DEV), space, route = 'long')
	assert forced[0].shape == (B, 2) and torch.equal(short[0], forced[0]) and torch.equal(short[1], forced[1])


def test_envelope_and_the_workspace_cap():
	from convasr_amd import _lib, ops
	one = torch.ones(1, dtype = torch.int32, device = DEV)
	wide = torch.zeros(1, 131072, dtype = torch.int32, device = DEV)
	few = torch.zeros(1, 5, dtype = torch.int32, device = DEV)
	with pytest.raises(_lib.ConvasrHipError, match = '131071'):
		ops.nw_align_long(wide, one, few, one, A.CHAR_SCORES)
	with pytest.raises(_lib.ConvasrHipError, match = '131071'):
		ops.edit_distance_long(few, one, wide, one)
	with pytest.raises(_lib.ConvasrHipError, match = '2048'):
		ops.nw_align_long(few, one, few, one, (2049, 0, 0, 0))
	with pytest.raises(_lib.ConvasrHipError):
		ops.nw_align_long(few.cpu(), one, few, one, A.CHAR_SCORES)
	T = tile()
	rng = random.Random(29)
	pairs = [(seq(rng, rng.randrange(0, 150), 3), seq(rng, rng.randrange(0, 150), 3)) for _ in range(60)] + [(seq(rng, 2 * T + 9, 3), seq(rng, 3 * T - 2, 3))]
	rng.shuffle(pairs)
	whole, whole_d = check_align(pairs, A.CHAR_SCORES), check_distance(pairs)
	cap = 3 * ops.nw_align_long_workspace_bytes(1, 2 * T + 9, 3 * T - 2)
	cap_d = 3 * ops.edit_distance_long_workspace_bytes(1, 2 * T + 9, 3 * T - 2)
	assert ops.nw_align_long_workspace_bytes(len(pairs), 2 * T + 9, 3 * T - 2) > cap and ops.edit_distance_long_workspace_bytes(len(pairs), 2 * T + 9, 3 * T - 2) > cap_d
	launches, real = [], ops.call
	ops.call = lambda name, *args: (launches.append(name), real(name, *args))[1]
	try:
		split = ops.nw_align_long(*pack(pairs), A.CHAR_SCORES, workspace_cap = cap)
		n_align = len(launches)
		split_d = ops.edit_distance_long(*pack(pairs), workspace_cap = cap_d)
	finally:
		ops.call = real
	assert 2 <= n_align < 20 and 2 <= len(launches) - n_align < 20
	assert set(launches[:n_align]) == {'convasr_nw_align_long_parts'} and set(launches[n_align:]) == {'convasr_edit_distance_long'}
	assert all(torch.equal(x, y) for x, y in zip(whole, split)) and torch.equal(whole_d, split_d)
	with pytest.raises(_lib.ConvasrHipError, match = 'nw_align_long'):
		ops.nw_align_long(*pack(pairs), A.CHAR_SCORES, workspace_cap = cap // 3 - 1)
	with pytest.raises(_lib.ConvasrHipError, match = 'edit_distance_long'):
		ops.edit_distance_long(*pack(pairs), workspace_cap = cap_d // 3 - 1)
