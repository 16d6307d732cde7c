"""ctc.star_alignment: the best path of a partial transcript through a whole recording (include/convasr_hip.h: convasr_star_alignment),
one wave per tile of the star lattice and one launch per anti-diagonal of tiles.

The rule is max and one rounded float32 addition per step, so every comparison with the float32 numpy restatement
(tests/_star_align_ref.py) is exact equality -- of the integer outputs and of the score's bits -- and so is every comparison with the
planted positions of inputs whose best path is known."""
import types

import numpy as np
import pytest
import torch

import _ctc_align_ref as R
import _star_align_ref as A

pytestmark = pytest.mark.gpu
C = 38
BLANK = C - 1
SPACE = 36  # CharTokenizerLegacy's space among 38 classes


def gpu(lp_tbc, tg, il, tl, mask, penalty, enter, **kwargs):
	import convasr_amd as ca
	r = ca.ctc.star_alignment(torch.as_tensor(lp_tbc).to('cuda:0'), torch.as_tensor(tg), torch.as_tensor(il), torch.as_tensor(tl), BLANK, torch.as_tensor(mask), penalty, enter, **kwargs)
	return types.SimpleNamespace(alignment = r.alignment.cpu().numpy(), star_begin = r.star_begin.cpu().numpy(), star_frames = r.star_frames.cpu().numpy(), score = r.score.cpu().numpy())


def same(x, y):
	return np.array_equal(x.alignment, y.alignment) and np.array_equal(x.star_begin, y.star_begin) and np.array_equal(x.star_frames, y.star_frames) and np.array_equal(x.score, y.score)


def check(lp, tg, il, tl, mask, penalty, enter, **kwargs):
	got = gpu(lp, tg, il, tl, mask, penalty, enter, **kwargs)
	want = A.align(np.asarray(lp), np.asarray(tg), np.asarray(il), np.asarray(tl), BLANK, np.asarray(mask), penalty, enter)
	assert got.score.dtype == np.float32 and got.alignment.dtype == np.int64 and got.star_begin.dtype == np.int64 and got.star_frames.dtype == np.int64
	assert same(got, want), (kwargs, np.asarray(tl).tolist(), np.asarray(il).tolist(), int((got.alignment != want.alignment).sum()), int((got.star_begin != want.star_begin).sum()),
	                         int((got.star_frames != want.star_frames).sum()), got.score.tolist(), want.score.tolist())
	return got


def gaps(tg, tl, mode):
	import convasr_amd as ca
	return ca.ctc.star_gaps(torch.as_tensor(tg), torch.as_tensor(tl), mode, SPACE).numpy()


def random_case(gen, T, S_max, il, tl, classes = C - 1):
	"""Random log-probs and random labels out of `classes` classes (few classes: repeats)."""
	return torch.randn(T, len(il), C, generator = gen).log_softmax(dim = -1).numpy(), torch.randint(0, classes, (len(il), S_max), generator = gen).numpy(), np.array(il), np.array(tl)


def worded_labels(seed, S, every = 6):
	"""S labels, letters with a space before every `every`-th one."""
	labels = np.random.RandomState(seed).randint(0, 33, size = S).astype(np.int64)
	labels[every - 1::every] = SPACE
	return labels


def planted_batch(seeds, T, labels, inserts, input_lengths):
	parts = [A.planted(seed, T, y, C, BLANK, ins, input_length = n) for seed, y, ins, n in zip(seeds, labels, inserts, input_lengths)]
	tg = np.zeros((len(parts), max(len(y) for y in labels)), dtype = np.int64)
	for b, y in enumerate(labels):
		tg[b, :len(y)] = y
	return np.stack([p[0] for p in parts], axis = 1), tg, np.array(input_lengths), np.array([len(y) for y in labels]), [p[1] for p in parts], [p[2] for p in parts]


def assert_planted(got, pos, runs):
	for b, (p, r) in enumerate(zip(pos, runs)):
		assert np.array_equal(got.alignment[b, :len(p)], p) and not got.alignment[b, len(p):].any(), (b, int((got.alignment[b, :len(p)] != p).sum()))
		for g in range(got.star_begin.shape[1]):
			assert (got.star_begin[b, g], got.star_frames[b, g]) == (r[g] if g in r else (-1, 0)), (b, g, got.star_begin[b, g], got.star_frames[b, g])
		assert np.isfinite(got.score[b])


def test_block_edges():
	"""2 n_units + 1 on either side of one and two blocks of states with a star in every gap, at the smallest chunk: T = 40 (three chunks:
	every state a path would have to end in lies past 4t + 3, so no row has a path and every carried read is the substituted -inf) and
	T = 320 (twenty chunks: paths exist -- also where equal neighbours need a frame between them -- and random frames favour the stars,
	so they take the s - 3 and s - 4 arcs across the block edges).  Rows of different
	lengths; what lies behind input_lengths[b] is then overwritten and nothing may change."""
	import convasr_amd as ca
	sb, _ = ca.ops.star_alignment_tiles()
	gen = torch.Generator().manual_seed(11)
	sizes = sorted({(L - 3) // 4 for k in (1, 2) for L in range(k * sb - 6, k * sb + 7) if (L - 3) % 4 == 0})
	assert len(sizes) >= 6
	for S in sizes:
		for T, il in ((40, [40, 33, 17]), (320, [320, 266, 70])):
			for classes, masks in ((C - 1, ('all', )), (3, ('all', 'odd'))):
				lp, tg, il_, tl = random_case(gen, T, S, il, [S, S - 1, S - 3], classes)
				for mode in masks:
					mask = gaps(tg, tl, 'all')
					if mode == 'odd':  # the units shift by one against the block edge
						mask[:, 0::2] = False
					got = check(lp, tg, il_, tl, mask, -0.7, -1.3, chunk_frames = 16)
					assert T == 40 or np.isfinite(got.score[:2]).all()
					dirty = lp.copy()
					for b, n in enumerate(il):
						dirty[n:, b] = 3.0
					assert same(gpu(dirty, tg, il_, tl, mask, -0.7, -1.3, chunk_frames = 16), got)


def test_chunk_edges():
	import convasr_amd as ca
	_, ch = ca.ops.star_alignment_tiles()
	gen = torch.Generator().manual_seed(12)
	for T in (15, 16, 17, 31, 32, 33):
		for S in (6, 40):  # (40 labels have no path through so few frames: -inf all the same)
			lp, tg, il, tl = random_case(gen, T, S, [T, T - 1], [S, S - 2])
			tg[:, 2::4] = SPACE
			check(lp, tg, il, tl, gaps(tg, tl, 'words'), -0.7, -1.3, chunk_frames = 16)
	for T in (ch - 1, ch, ch + 1):
		lp, tg, il, tl = random_case(gen, T, 40, [T, T - 1], [40, 37])
		tg[:, 2::4] = SPACE
		got = check(lp, tg, il, tl, gaps(tg, tl, 'words'), -0.7, -1.3)
		assert np.isfinite(got.score).all()


@pytest.fixture(scope = 'module')
def cut_batch():
	labels = [worded_labels(21, 700), worded_labels(22, 640)]
	return planted_batch((21, 22), 3000, labels, [{100: 200, 401: 150}, {0: 120, 640: 90}], [3000, 2700])


def test_result_does_not_depend_on_the_cut(cut_batch):
	"""700 labels over 3,000 frames, a star in every gap, at chunk lengths 16, 64 and the default: one result, the restatement's, the planted one."""
	lp, tg, il, tl, pos, runs = cut_batch
	mask = gaps(tg, tl, 'all')
	first = check(lp, tg, il, tl, mask, -1.0, -2.0, chunk_frames = 16)
	assert_planted(first, pos, runs)
	for chunk_frames in (64, 0):
		assert same(gpu(lp, tg, il, tl, mask, -1.0, -2.0, chunk_frames = chunk_frames), first), chunk_frames


def test_finds_the_audio_the_transcript_skips():
	"""120 labels in two stretches around 300 frames of foreign speech, stars before the words: the star of that gap takes exactly the
	insert, no other star is used, every label sits on its frame -- and ctc.alignment_long, which has no star, moves labels off theirs."""
	import convasr_amd as ca
	labels = worded_labels(31, 120)
	gap = 65
	assert labels[gap] == SPACE
	lp, pos, runs = A.planted(31, 1200, labels, C, BLANK, {gap: 300})
	tg, il, tl = labels[None], np.array([1200]), np.array([120])
	mask = gaps(tg, tl, 'words')
	assert mask[0, gap] and 10 < mask.sum() < 40
	got = check(lp[:, None], tg, il, tl, mask, -1.0, -2.0)
	assert (got.star_begin[0, gap], got.star_frames[0, gap]) == runs[gap] and runs[gap][1] == 300
	assert_planted(got, [pos], [runs])
	plain = ca.ctc.alignment_long(torch.from_numpy(lp[:, None]).to('cuda:0'), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl), blank = BLANK).cpu().numpy()
	assert (plain[0] != pos).any()
	# StarCTC.align on the model's layout is the same call
	star = ca.ctc.StarCTC('words', penalty = -1.0, enter = -2.0, space = SPACE)
	r = star.align(torch.from_numpy(lp[None]).to('cuda:0').permute(0, 2, 1), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl), BLANK)
	assert np.array_equal(r.alignment.cpu().numpy(), got.alignment) and np.array_equal(r.star_frames.cpu().numpy(), got.star_frames) and np.array_equal(r.score.cpu().numpy(), got.score)


def test_all_false_mask_is_alignment_long():
	import convasr_amd as ca
	sb, ch = ca.ops.star_alignment_tiles()
	for seeds, T, labels, lengths in (((1, 2), 2 * ch + 1, [sb // 2, sb // 2 - 1], [2 * ch + 1, 2 * ch]), ((3, 4, 5), 6 * sb + 7, [sb + sb // 2, sb, 1], [6 * sb + 7, 5 * sb, 4])):
		parts = [R.planted(seed, T, S, C, BLANK, 12.0, input_length = n) for seed, S, n in zip(seeds, labels, lengths)]
		tg = np.zeros((len(parts), max(labels)), dtype = np.int64)
		for b, (_, t, _) in enumerate(parts):
			tg[b, :len(t)] = t
		lp, il, tl = np.stack([p[0] for p in parts], axis = 1), np.array(lengths), np.array(labels)
		got = check(lp, tg, il, tl, np.zeros((len(parts), max(labels) + 1), dtype = bool), -1.0, -2.0)
		plain = ca.ctc.alignment_long(torch.from_numpy(lp).to('cuda:0'), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl), blank = BLANK).cpu().numpy()
		assert np.array_equal(got.alignment, plain)
		assert_planted(got, [p[2] for p in parts], [{}] * len(parts))


def test_size():
	"""3,000 labels over 12,000 frames with four inserts: the planted positions (the restatement is too slow here)."""
	labels = worded_labels(41, 3000)
	lp, tg, il, tl, pos, runs = planted_batch((41, ), 12000, [labels], [{0: 400, 1001: 700, 2500: 350, 3000: 500}], [11990])
	got = gpu(lp, tg, il, tl, gaps(tg, tl, 'all'), -1.0, -2.0)
	assert_planted(got, pos, runs)
	again = gpu(lp, tg, il, tl, gaps(tg, tl, 'words'), -1.0, -2.0)  # (gaps 0 and 3,000 are ends; 1,001 and 2,500 are no word gaps: other cases, same labels)
	assert np.isfinite(again.score[0]) and again.score[0] < got.score[0]
	assert (again.star_begin[0, 0], again.star_frames[0, 0]) == runs[0][0] and (again.star_begin[0, 3000], again.star_frames[0, 3000]) == runs[0][3000]


def test_edge_cases():
	gen = torch.Generator().manual_seed(13)
	# rows without a path (too few frames, no frames, more frames than the batch has) among rows with one; a padded S_max
	lp, tg, il, tl = random_case(gen, 30, 25, [30, 3, 0, 31, 30, 30, 1, 1, 1], [12, 10, 4, 4, 0, 0, 1, 0, 2], 3)
	mask = gaps(tg, tl, 'all')
	mask[5] = False  # no label and no star: one blank state
	mask[6] = False
	got = check(lp, tg, il, tl, mask, -0.7, -1.3)
	assert np.isfinite(got.score).tolist() == [True, False, False, False, True, True, True, True, False]
	assert got.star_frames[4, 0] == 30 and got.star_begin[4, 0] == 0 and not got.alignment[4:6].any()  # the star beats thirty random blanks
	assert got.star_frames[5].sum() == 0 and got.alignment[6, 0] == 0
	for b in (1, 2, 3, 8):
		assert not got.alignment[b].any() and (got.star_begin[b] == -1).all() and not got.star_frames[b].any() and got.score[b] == -np.inf
	assert same(gpu(lp, tg, il, tl, mask, -0.7, -1.3), got)  # two runs: the same bits
	# B = 1, and S_max = 0
	check(lp[:, :1], tg[:1], il[:1], tl[:1], mask[:1], -0.7, -1.3, chunk_frames = 16)
	check(lp[:, 4:6], tg[4:6, :0], il[4:6], tl[4:6], mask[4:6, :1], -0.7, -1.3)
	# costs of zero are legal
	check(lp, tg, il, tl, mask, 0.0, 0.0)


def test_errors():
	import convasr_amd as ca
	from convasr_amd import _lib
	d = torch.device('cuda:0')
	lp, tg, il, tl = torch.zeros(1, 50, C, device = d), torch.zeros(1, 20, dtype = torch.int64), torch.tensor([50]), torch.tensor([20])
	mask = torch.ones(1, 21, dtype = torch.bool)
	assert ca.ops.star_ctc_alignment(lp, tg, il, tl, BLANK, mask, -1.0, -2.0).alignment.shape == (1, 20)
	for kw in (dict(star_penalty = 0.5), dict(star_enter = 0.25), dict(star_mask = mask[:, :20]), dict(chunk_frames = 8)):
		with pytest.raises((ValueError, _lib.ConvasrHipError)):
			ca.ops.star_ctc_alignment(**dict(dict(log_probs_btc = lp, targets = tg, input_lengths = il, target_lengths = tl, blank = BLANK, star_mask = mask, star_penalty = -1.0, star_enter = -2.0), **kw))
	big = torch.zeros(1, 4000, C, device = d)
	with pytest.raises(_lib.ConvasrHipError, match = 'bytes of workspace'):
		ca.ops.star_ctc_alignment(big, torch.zeros(1, 1500, dtype = torch.int64), torch.tensor([4000]), torch.tensor([1500]), BLANK, torch.ones(1, 1501, dtype = torch.bool), -1.0, -2.0, workspace_cap = 1 << 20)


def test_transcribe_batch_with_a_star():
	"""transcribe_batch with args.align_star: alignment, star_segments and ref_pieces are ops.star_ctc_alignment's on out.log_probs; without
	the attribute the alignment is ctc.alignment_bct's and the new fields are None."""
	import convasr_amd as ca
	from convasr_amd.transcript_generators import CharTokenizerLegacy, GreedyCTCGenerator
	d = torch.device('cuda:0')
	tokenizer = CharTokenizerLegacy(ca.transcribe.RU_ALPHABET)
	assert tokenizer.vocab_size == C and tokenizer.eps_id == BLANK and tokenizer.space_id == SPACE
	labels = [worded_labels(51, 60), worded_labels(52, 48)]
	lp, tg, il, tl, pos, runs = planted_batch((51, 52), 400, labels, [{17: 80, 41: 3}, {48: 40}], [400, 380])
	tg, il, tl = torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)
	assert labels[0][17] == SPACE and labels[0][41] == SPACE
	log_probs = torch.from_numpy(lp).permute(1, 0, 2).contiguous().to(d).permute(0, 2, 1)  # logical (B, C, T), memory (B, T, C)
	model = lambda x, xlen: (log_probs, log_probs, il.to(d))
	star = ca.ctc.StarCTC('words', penalty = -1.0, enter = -2.0, space = SPACE)
	B = 2
	batch = (torch.zeros(B, 1, 8000 * 8), torch.ones(B), torch.zeros(B), torch.full((B, ), 8.0))
	run = lambda args: ca.transcribe.transcribe_batch(args, ca.transcribe.TextPipeline(tokenizer), model, GreedyCTCGenerator(), *batch, y = tg.unsqueeze(1), ylen = tl.unsqueeze(1))
	out = run(types.SimpleNamespace(device = 'cuda:0', sample_rate = 8000, align = True, align_star = star, align_star_min_frames = 10))
	direct = ca.ops.star_ctc_alignment(out.log_probs.permute(0, 2, 1).contiguous(), tg, il, tl, BLANK, star.mask(tg, tl), -1.0, -2.0)
	assert torch.equal(out.alignment, direct.alignment)
	assert_planted(types.SimpleNamespace(alignment = direct.alignment.cpu().numpy(), star_begin = direct.star_begin.cpu().numpy(), star_frames = direct.star_frames.cpu().numpy(), score = direct.score.cpu().numpy()), pos, runs)
	ts = out.ts.cpu()
	pieces = ca.ctc.star_pieces(direct, tg, tl, 10)
	assert [[(s['gap'], s['frames']) for s in segs] for segs in out.star_segments] == [[(17, 80)], [(48, 40)]]  # (the 3-frame star is under align_star_min_frames)
	for b in range(B):
		assert [(s['gap'], s['begin'], s['end'], s['frames']) for s in out.star_segments[b]] == [(g, float(ts[b, lo]), float(ts[b, hi]), hi - lo + 1) for g, lo, hi in pieces[b].stars]
		assert [(p['first_label'], p['label_count'], p['begin'], p['end']) for p in out.ref_pieces[b]] == [(first, count, float(ts[b, lo]), float(ts[b, hi])) for first, count, lo, hi in pieces[b].pieces]
	assert [(p['first_label'], p['label_count']) for p in out.ref_pieces[0]] == [(0, 17), (17, 43)] and [(p['first_label'], p['label_count']) for p in out.ref_pieces[1]] == [(0, 48)]
	assert len(out.ref_segments) == B and all(len(r) >= 8 for r in out.ref_segments)
	short = run(types.SimpleNamespace(device = 'cuda:0', sample_rate = 8000, align = True, align_star = star))
	assert [[s['gap'] for s in segs] for segs in short.star_segments] == [[17, 41], [48]]
	plain = run(types.SimpleNamespace(device = 'cuda:0', sample_rate = 8000, align = True))
	assert plain.star_segments is None and plain.ref_pieces is None
	assert torch.equal(plain.alignment, ca.ctc.alignment_bct(log_probs, tg, il, tl, blank = BLANK)) and len(plain.ref_segments) == B
	assert torch.equal(plain.log_probs, out.log_probs) and plain.hyp == out.hyp
