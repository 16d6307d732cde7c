"""ctc.alignment_long: forced alignment of whole recordings (up to 131,071 labels over 2^20 frames) on many compute units, one wave per tile
of the lattice and one launch per anti-diagonal of tiles (include/convasr_hip.h: convasr_ctc_alignment_long).

Every comparison is exact equality of integer tensors: against ctc.alignment (the one-wave and one-workgroup kernels) wherever that
takes the targets, against the reference's golden arrays, against the numpy restatement of the reference (tests/_ctc_align_ref.py) and
against the planted positions of inputs whose best path is known."""
import os
import re
import types

import numpy as np
import pytest
import torch

import _ctc_align_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C = 38


def both(lp, tg, il, tl, blank, **kwargs):
	"""(alignment_long, alignment) of one batch, on the CPU."""
	import convasr_amd as ca
	d = torch.device('cuda:0')
	lp = lp.to(d)
	return ca.ctc.alignment_long(lp, tg, il, tl, blank = blank, **kwargs).cpu(), ca.ctc.alignment(lp, tg, il, tl, blank = blank).cpu()


def random_case(gen, T, S_max, il, tl):
	return torch.randn(T, len(il), C, generator = gen).log_softmax(dim = -1), torch.randint(0, C - 1, (len(il), S_max), generator = gen), torch.tensor(il), torch.tensor(tl)


def planted_batch(seeds, T, labels, input_lengths, boost = 12.0):
	"""(log_probs (T, B, C), targets (B, max labels) zero-padded, input_lengths, target_lengths, [pos per utterance])."""
	parts = [R.planted(seed, T, S, C, C - 1, boost, input_length = n) for seed, S, n in zip(seeds, labels, input_lengths)]
	tg = torch.zeros(len(parts), max(labels), dtype = torch.int64)
	for b, (_, t, _) in enumerate(parts):
		tg[b, :len(t)] = torch.from_numpy(t)
	return torch.from_numpy(np.stack([p[0] for p in parts], axis = 1)), tg, torch.tensor(input_lengths), torch.tensor(labels), [p[2] for p in parts]


def test_equals_the_existing_kernels_and_the_golden_arrays():
	g0, g1 = np.load(os.path.join(GOLDEN, 'alignment.npz')), np.load(os.path.join(GOLDEN, 'alignment_long.npz'))
	keys = ('log_probs', 'targets', 'input_lengths', 'target_lengths', 'alignment')
	cases = [tuple(torch.from_numpy(g0[f'c{c}/{k}']) for k in keys) + (int(g0[f'c{c}/blank']), ) for c in (0, 1, 2)]
	cases.append(tuple(torch.from_numpy(g1[k]) for k in keys) + (int(g1['blank']), ))
	# the 64 x 753 x 150 batch and the ragged 2,100-label / 6,000-frame case of test_ctc_alignment_of_long_targets_and_the_two_kernels_agree
	gen = torch.Generator().manual_seed(8)
	B, T, S = 64, 753, 150
	cases.append((torch.randn(T, B, C, generator = gen).log_softmax(dim = -1), torch.randint(0, C - 1, (B, S), generator = gen), torch.randint(2 * S + 1, T + 1, (B, ), generator = gen), torch.randint(1, S + 1, (B, ), generator = gen), None, C - 1))
	B, T, S = 2, 6000, 2100
	tg = torch.randint(0, C - 1, (B, S), generator = gen)
	tl, il = torch.tensor([S, 1500]), torch.tensor([T, 5000])
	logits = torch.randn(T, B, C, generator = gen)
	for b in range(B):
		pos = (torch.arange(int(tl[b])) * (int(il[b]) - 10) / int(tl[b])).long() + 3
		logits[pos, b, tg[b, :int(tl[b])]] += 6.0
	cases.append((logits.log_softmax(dim = -1), tg, il, tl, None, C - 1))
	for k, (lp, tg, il, tl, golden, blank) in enumerate(cases):
		long, short = both(lp, tg, il, tl, blank)
		assert torch.equal(long, short), (k, int((long != short).sum()))
		assert golden is None or torch.equal(long, golden), (k, int((long != golden).sum()))


def test_tile_edges():
	"""2 S + 1 on either side of a multiple of the states of a block (and on it, where that is odd), T on either side of the chunk length and
	on it, T shorter than a chunk, one label, one frame, padded recordings, padded targets, no target, more labels than frames (no
	path: the existing kernels' answer all the same), and batches that mix them."""
	import convasr_amd as ca
	sb, chunk = ca.ops.ctc_alignment_long_tiles()
	gen = torch.Generator().manual_seed(31)
	cases = []
	for k in (1, 2, 3):
		for L in (k * sb - 1, k * sb, k * sb + 1):
			if L % 2 == 1:
				S = (L - 1) // 2
				cases.append(random_case(gen, 2 * chunk + 5, S, [2 * chunk + 5], [S]))
	for T in (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1):
		cases.append(random_case(gen, T, sb, [T], [sb]))  # (three blocks; more labels than frames at the short ones)
		cases.append(random_case(gen, T, chunk // 4, [T], [chunk // 4]))
	cases.append(random_case(gen, 7, 3, [7], [3]))
	cases.append(random_case(gen, 1, 1, [1], [1]))
	cases.append(random_case(gen, 100, 300, [100], [300]))
	cases.append(random_case(gen, chunk + 3, 1, [chunk + 3], [1]))
	cases.append(random_case(gen, 3 * chunk, sb // 2 + 40, [2 * chunk - 1], [sb // 2 - 1]))
	T, S_max = 2 * chunk + 1, sb + 10
	cases.append(random_case(gen, T, S_max, [T, chunk, chunk + 1, T - 1, 5, T, T], [S_max, 1, sb // 2 - 1, sb // 2, 77, 0, sb // 2 + 1]))
	for k, (lp, tg, il, tl) in enumerate(cases):
		for chunk_frames in (0, 16):
			long, short = both(lp, tg, il, tl, C - 1, chunk_frames = chunk_frames)
			assert torch.equal(long, short), (k, chunk_frames, lp.shape, tl.tolist(), il.tolist(), int((long != short).sum()))
	# planted recordings that straddle the same edges, against the restatement and the planted positions
	for seeds, T, labels, lengths in (((1, 2), 2 * chunk + 1, [sb // 2, sb // 2 - 1], [2 * chunk + 1, 2 * chunk]), ((3, 4, 5), 6 * sb + 7, [sb + sb // 2, sb, 1], [6 * sb + 7, 5 * sb, 4])):
		lp, tg, il, tl, pos = planted_batch(seeds, T, labels, lengths)
		long, short = both(lp, tg, il, tl, C - 1)
		assert torch.equal(long, short)
		assert np.array_equal(long.numpy(), R.alignment(lp.numpy(), tg.numpy(), il.numpy(), tl.numpy(), blank = C - 1))
		for b, p in enumerate(pos):
			assert np.array_equal(long[b, :len(p)].numpy(), p) and not long[b, len(p):].any()


def test_result_does_not_depend_on_the_cut():
	"""3,000 labels over 9,000 frames at the smallest legal chunk, the default and a long one: one result, ctc.alignment's."""
	gen = torch.Generator().manual_seed(41)
	lp, tg, il, tl = random_case(gen, 9000, 3000, [9000, 8000], [3000, 2800])
	results = [both(lp, tg, il, tl, C - 1, chunk_frames = chunk_frames) for chunk_frames in (16, 0, 1000)]
	for long, short in results:
		assert torch.equal(long, results[0][0]) and torch.equal(long, short)


@pytest.fixture(scope = 'module')
def past_the_old_envelope():
	return planted_batch((11, 12), 24000, [9000, 8500], [24000, 23000])


def test_past_the_old_envelope(past_the_old_envelope):
	"""9,000 and 8,500 labels over 24,000 frames -- ctc.alignment refuses more than 8,191: the restatement's path, which is the planted one."""
	import convasr_amd as ca
	lp, tg, il, tl, pos = past_the_old_envelope
	al = ca.ctc.alignment_long(lp.to('cuda:0'), tg, il, tl, blank = C - 1).cpu().numpy()
	ref = R.alignment(lp.numpy(), tg.numpy(), il.numpy(), tl.numpy(), blank = C - 1)
	assert np.array_equal(al, ref), int((al != ref).sum())
	for b, p in enumerate(pos):
		assert np.array_equal(al[b, :len(p)], p), (b, int((al[b, :len(p)] != p).sum()))
		assert not al[b, len(p):].any()


def test_one_hour():
	"""48,000 labels over 180,000 frames (an hour of telephone speech at 50 encoder frames a second): the planted positions."""
	import convasr_amd as ca
	T, S, Tb = 180000, 48000, 179500
	lp, tg, pos = R.planted(7, T, S, C, C - 1, 12.0, input_length = Tb)
	al = ca.ctc.alignment_long(torch.from_numpy(lp).unsqueeze(1).to('cuda:0'), torch.from_numpy(tg).unsqueeze(0), torch.tensor([Tb]), torch.tensor([S]), blank = C - 1).cpu().numpy()[0]
	assert np.array_equal(al, pos), int((al != pos).sum())
	assert bool((al[1:] > al[:-1]).all()) and int(al.max()) < Tb


def test_errors():
	import convasr_amd as ca
	from convasr_amd import _lib
	d = torch.device('cuda:0')
	lp = torch.zeros(50, 1, C, device = d)
	need = _lib.load().convasr_ctc_alignment_long_workspace_bytes(1, 50, 20)
	with pytest.raises(_lib.ConvasrHipError, match = f'{need} bytes'):
		ca.ops.ctc_alignment_long(lp.permute(1, 0, 2).contiguous(), torch.zeros(1, 20, dtype = torch.int64), torch.tensor([50]), torch.tensor([20]), C - 1, workspace_cap = need - 1)
	assert ca.ops.ctc_alignment_long(lp.permute(1, 0, 2).contiguous(), torch.zeros(1, 20, dtype = torch.int64), torch.tensor([50]), torch.tensor([20]), C - 1, workspace_cap = need).shape == (1, 20)
	with pytest.raises(_lib.ConvasrHipError, match = 'target length 131072 > 131071'):
		ca.ctc.alignment_long(torch.zeros(4, 1, C, device = d), torch.zeros(1, 131072, dtype = torch.int64), torch.tensor([4]), torch.tensor([1]), blank = C - 1)
	with pytest.raises(_lib.ConvasrHipError, match = 'chunk_frames'):
		ca.ctc.alignment_long(lp, torch.zeros(1, 20, dtype = torch.int64), torch.tensor([50]), torch.tensor([20]), blank = C - 1, chunk_frames = 8)


def test_transcribe_batch_aligns_a_whole_recording(past_the_old_envelope):
	"""transcribe_batch with args.align and 9,000 target labels: the alignment of ctc.alignment_long_bct, one ref segment per word."""
	import convasr_amd as ca
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	d = torch.device('cuda:0')
	lp, tg, il, tl, pos = past_the_old_envelope
	tokenizer = CharTokenizerLegacy(ca.transcribe.RU_ALPHABET)
	assert tokenizer.vocab_size == C and tokenizer.eps_id == C - 1
	log_probs = lp.permute(1, 0, 2).contiguous().to(d).permute(0, 2, 1)  # logical (B, C, T), memory (B, T, C)
	model = lambda x, xlen: (log_probs, log_probs, il.to(d))
	args = types.SimpleNamespace(device = 'cuda:0', sample_rate = 8000, align = True)
	B = len(il)
	out = ca.transcribe.transcribe_batch(args, ca.transcribe.TextPipeline(tokenizer), model, GreedyCTCGenerator(), torch.zeros(B, 1, 8000 * 480), torch.ones(B), torch.zeros(B), torch.full((B, ), 480.0),
	                                     y = tg.unsqueeze(1), ylen = tl.unsqueeze(1))
	direct = ca.ctc.alignment_long_bct(log_probs, tg, il, tl, blank = tokenizer.eps_id)
	assert out.alignment.shape == tg.shape and torch.equal(out.alignment, direct)
	for b in range(B):
		text = tokenizer.decode([tg[b, :int(tl[b])].tolist()])[0]
		words = 1 + len(re.findall(' +', text.lstrip(' ')))  # a segment opens at the first character and at every run of spaces
		assert words > 100 and len(out.ref_segments[b]) == words, (b, words, len(out.ref_segments[b]))
		begins = [s['begin'] for s in out.ref_segments[b]]
		assert all(x <= y for x, y in zip(begins, begins[1:]))
