"""Character and word error rates (reference: metrics.py:409-421, cer / wer) with the edit distances on the GPU (convasr_edit_distance; past
16,383 units a side, a whole recording, convasr_edit_distance_long -- and convasr_nw_align_long for the alignments below).

Two paths:
* strings -- cer / wer / cer_wer: the reference's arithmetic exactly.  CER compares hyp.replace(' ', '').lower() with the same of ref
  (only U+0020 is removed) over Unicode codepoints and divides by len(ref.replace(' ', '')) or 1 of the ref as given (lowercasing can
  change a length: 'İ'.lower() is two codepoints).  WER splits both sides on any whitespace, without lowercasing, maps the words to
  integer ids on the host (the reference's word2char) and divides by len(ref.split()) or 1.  hyp == ref scores 0.  The host prepares
  codepoints / word ids; one launch per metric computes every distance; the ratio is a float64 division of the two integers, as Python's
  int / int is.
* tokens -- token_cer_wer: device tensors of token ids in, device tensors of per-utterance rates out, no host round trip.  It is valid for a
  tokenizer in which every class decodes to one character c with c.lower() == c and only the space class decodes to whitespace
  (CharTokenizerLegacy with the Russian alphabet is one): there it equals the string path applied to tokenizer.decode of the same tokens.
  For any other tokenizer (BPE) decode the tokens and use the string path."""
import collections
import math

import numpy as np
import torch

from . import _lib, ops


def _device(device):
	return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def _pack(seqs, device):
	"""Lists of ints -> (N, L) int64 device tensor (zero-padded, L >= 1) and (N,) int64 lengths, one host-to-device copy each."""
	L = max([len(s) for s in seqs] + [1])
	arr = np.zeros((len(seqs), L), dtype = np.int64)
	for i, s in enumerate(seqs):
		arr[i, :len(s)] = s
	lengths = np.array([len(s) for s in seqs], dtype = np.int64)
	return torch.from_numpy(arr).to(device), torch.from_numpy(lengths).to(device)


def char_units(hyps, refs):
	"""The CER inputs of the reference's cer: per pair the codepoints of hyp.replace(' ', '').lower() and of ref.replace(' ', '').lower(), and
	the denominator len(ref.replace(' ', '')) or 1 (before lowercasing)."""
	h = [[ord(c) for c in s.replace(' ', '').lower()] for s in hyps]
	r = [[ord(c) for c in s.replace(' ', '').lower()] for s in refs]
	return h, r, [len(s.replace(' ', '')) or 1 for s in refs]


def word_units(hyps, refs):
	"""The WER inputs of the reference's wer: per pair the word ids of hyp.split() and ref.split() (equal words, equal ids), and the
	denominator len(ref.split()) or 1."""
	ids = {}
	h = [[ids.setdefault(w, len(ids)) for w in s.split()] for s in hyps]
	r = [[ids.setdefault(w, len(ids)) for w in s.split()] for s in refs]
	return h, r, [len(s.split()) or 1 for s in refs]


def split_route(len_a, len_b, route = None):
	"""Which pairs take which kernels: (short, long) lists of pair numbers.  route None: a pair whose unit counts both fit
	_lib.METRIC_MAX_LEN = 16,383 (the envelope of ops.edit_distance / ops.nw_align) is short, the others are long (the tiled
	ops.edit_distance_long / ops.nw_align_long, up to 131,071 units a side); 'short' / 'long' send every pair one way (tests and timing)."""
	if route not in (None, 'short', 'long'):
		raise ValueError(f"route {route!r} is not None, 'short' or 'long'")
	fits = [route == 'short' or (route is None and max(m, n) <= _lib.METRIC_MAX_LEN) for m, n in zip(len_a, len_b)]
	return [p for p, f in enumerate(fits) if f], [p for p, f in enumerate(fits) if not f]


def _pack32(seqs, device):
	"""_pack for the long route: int32 ids."""
	t, lengths = _pack(seqs, device)
	return t.to(torch.int32), lengths.to(torch.int32)


def _distances(hyp_units, ref_units, device, route = None, short_fn = None, long_fn = None):
	"""The edit distance of every pair, as a list: the short pairs in one ops.edit_distance call (the only call when every pair is short),
	the long ones in one ops.edit_distance_long call."""
	short_fn, long_fn = short_fn or ops.edit_distance, long_fn or ops.edit_distance_long
	short, long = split_route([len(h) for h in hyp_units], [len(r) for r in ref_units], route)
	dist = [0] * len(hyp_units)
	if short:
		h, hl = _pack([hyp_units[p] for p in short], device)
		r, rl = _pack([ref_units[p] for p in short], device)
		for p, d in zip(short, short_fn(h, hl, r, rl, _lib.METRIC_CHARS, -1)[0].cpu().tolist()):
			dist[p] = d
	if long:
		h, hl = _pack32([hyp_units[p] for p in long], device)
		r, rl = _pack32([ref_units[p] for p in long], device)
		for p, d in zip(long, long_fn(h, hl, r, rl).cpu().tolist()):
			dist[p] = d
	return dist


def _rates(hyp_units, ref_units, denominators, equal, device, route = None):
	return [0.0 if same else d / n for d, n, same in zip(_distances(hyp_units, ref_units, device, route), denominators, equal)]


def cer_wer(hyps, refs, device = None, route = None):
	"""Per-utterance CER and WER of the string pairs (hyps[i], refs[i]), as the reference's metrics.cer / metrics.wer compute them:
	two lists of floats.  Pairs of at most 16,383 units a side run on ops.edit_distance, longer ones (a whole recording: up to 131,071
	units a side) on ops.edit_distance_long; route forces one of the two (split_route)."""
	hyps, refs = list(hyps), list(refs)
	if len(hyps) != len(refs):
		raise ValueError(f'cer_wer: {len(hyps)} hypotheses for {len(refs)} references')
	if not hyps:
		return [], []
	device = _device(device)
	equal = [a == b for a, b in zip(hyps, refs)]
	return _rates(*char_units(hyps, refs), equal, device, route), _rates(*word_units(hyps, refs), equal, device, route)


def cer(*, hyp, ref):
	"""metrics.cer (metrics.py:409-411) for one pair, the distance computed on the GPU."""
	return cer_wer([hyp], [ref])[0][0]


def wer(*, hyp, ref):
	"""metrics.wer (metrics.py:414-421) for one pair, the distance computed on the GPU."""
	return cer_wer([hyp], [ref])[1][0]


def _compact_chars(tokens, lengths, space):
	"""(N, L) int64 tokens -> (the tokens below each length that are not `space`, moved to the front in order, as int32; their count (N,)
	int32), on the device: a stable sort of the keep mask."""
	L = tokens.shape[1]
	keep = (tokens != space) & (torch.arange(L, device = tokens.device)[None, :] < lengths[:, None])
	order = torch.sort((~keep).to(torch.uint8), dim = 1, stable = True).indices
	return tokens.gather(1, order).to(torch.int32), keep.sum(dim = 1).to(torch.int32)


def _word_id_rows(rows, lengths, space, ids):
	"""Host lists of tokens -> per row the ids of its maximal runs of non-space tokens (equal words, equal ids: a dict of tuples, exact)."""
	out = []
	for row, n in zip(rows, lengths):
		words, cur = [], []
		for t in row[:max(n, 0)] + [space]:
			if t != space:
				cur.append(t)
			elif cur:
				words.append(ids.setdefault(tuple(cur), len(ids)))
				cur = []
		out.append(words)
	return out


def _token_cer_wer_long(tokens, lengths, ref, ref_lengths, space):
	squeeze = tokens.ndim == 2
	if squeeze:
		tokens, lengths = tokens.unsqueeze(1), torch.as_tensor(lengths).unsqueeze(1)
	B, K, L = tokens.shape
	dev = tokens.device
	hyp = tokens.reshape(B * K, L)
	hl = torch.as_tensor(lengths).to(device = dev, dtype = torch.int64).reshape(B * K).clamp(0, L)
	rl = torch.as_tensor(ref_lengths).to(device = dev, dtype = torch.int64).clamp(0, ref.shape[1])
	pair_ref = torch.arange(B, device = dev).repeat_interleave(K)
	# CHARS: the non-space tokens, compacted on the device
	hc, hn = _compact_chars(hyp, hl, space)
	rc, rn = _compact_chars(ref, rl, space)
	cd = ops.edit_distance_long(hc, hn, rc[pair_ref], rn[pair_ref])
	# WORDS: word ids through a dict on the host (one round trip)
	ids = {}
	rw = _word_id_rows(ref.cpu().tolist(), rl.cpu().tolist(), space, ids)
	hw = _word_id_rows(hyp.cpu().tolist(), hl.cpu().tolist(), space, ids)
	hwt, hwl = _pack32(hw, dev)
	rwt, rwl = _pack32([rw[p // K] for p in range(B * K)], dev)
	wd = ops.edit_distance_long(hwt, hwl, rwt, rwl)
	units, words = rn.double().clamp(min = 1), torch.tensor([len(w) for w in rw], dtype = torch.float64, device = dev).clamp(min = 1)
	cer, wer = cd.double().view(B, K) / units.view(B, 1), wd.double().view(B, K) / words.view(B, 1)
	return (cer[:, 0], wer[:, 0]) if squeeze else (cer, wer)


def token_cer_wer(tokens, lengths, ref, ref_lengths, space, route = None):
	"""Per-utterance CER and WER of token hypotheses against token references, on the device.  tokens (B, K, L) int64 with lengths (B, K), or
	(B, L) with (B,); ref (B, Lr) int64 read in place through its row stride (y[:, 0]), ref_lengths (B,) (ylen[:, 0]); space: the space class.
	CER = edit distance over the tokens that are not `space` / (their number in the reference or 1); WER = edit distance over the maximal
	runs of non-space tokens / (their number in the reference or 1).  Returns two float64 device tensors shaped like lengths.  Valid for
	one-character lowercase tokenizers only (see the module docstring).

	While L and Lr are at most 16,383 (route None; 'short' forces it) ops.edit_distance makes the units itself and nothing leaves the
	device.  Longer batches (a whole recording; up to 131,071 units a side; 'long' forces it) go to ops.edit_distance_long, whose unit ids
	this function makes: the non-space tokens compacted on the device for CER, and for WER word ids through a dict on the HOST, which is
	exact and costs one round trip of the tokens (class ids must fit int32)."""
	if route not in (None, 'short', 'long'):
		raise ValueError(f"route {route!r} is not None, 'short' or 'long'")
	if route == 'long' or (route is None and max(tokens.shape[-1], ref.shape[-1]) > _lib.METRIC_MAX_LEN):
		ops.require_cuda(tokens, ref)
		return _token_cer_wer_long(tokens, lengths, ref, ref_lengths, int(space))
	cd, units = ops.edit_distance(tokens, lengths, ref, ref_lengths, _lib.METRIC_CHARS, int(space))
	wd, words = ops.edit_distance(tokens, lengths, ref, ref_lengths, _lib.METRIC_WORDS, int(space))
	shape = (-1, ) + (1, ) * (cd.ndim - 1)
	return cd.double() / units.clamp(min = 1).double().view(shape), wd.double() / words.clamp(min = 1).double().view(shape)


# ------------------------------------------------------------------------------------------------ alignment and error analysis
#
# The reference's align_strings / align_words / ErrorTagger / WordTagger / ErrorAnalyzer (metrics.py:17-232, 261-407) with its names, keyword
# arguments and result keys, so that configurations written for it work unchanged.  The quadratic part, the Needleman-Wunsch alignment, runs
# on the GPU (ops.nw_align); everything else is host string code that CONSUMES alignment results and scores: every function below takes an
# `aligner` and, where it needs error rates, a `scorer`, and defaults them to the GPU ones.
#   aligner(a_seqs, b_seqs, scores) -> per pair (a_index, b_index): lists of ints, one entry per alignment column, -1 for a gap
#   scorer(hyps, refs) -> (cers, wers): cer_wer's contract

placeholder = '|'
space = ' '
silence = placeholder + space

WORD_ALIGN_SCORES = (100, -6, -8, -3)  # (match, sub, del, ins), see align_strings
CHAR_ALIGN_SCORES = (5, -3, -4, -3)


def replace_placeholder(s, rep = ''):
	return s.replace(placeholder, rep)


def gpu_aligner(a_seqs, b_seqs, scores, device = None, route = None, short_fn = None, long_fn = None):
	"""The default aligner: all pairs in one ops.nw_align call, the index rows back in one device-to-host copy.  Pairs with more than
	16,383 units on a side (a whole recording; up to 131,071) go to ops.nw_align_long in a second call; route forces one of the two
	(split_route)."""
	if not a_seqs:
		return []
	device = _device(device)
	short, long = split_route([len(s) for s in a_seqs], [len(t) for t in b_seqs], route)
	out = [None] * len(a_seqs)
	for members, fn in ((short, short_fn or ops.nw_align), (long, long_fn or ops.nw_align_long)):
		if members:
			for p, cols in zip(members, _align_group(fn, [a_seqs[p] for p in members], [b_seqs[p] for p in members], scores, device)):
				out[p] = cols
	return out


def _align_group(nw_align, a_seqs, b_seqs, scores, device):
	N = len(a_seqs)
	La, Lb = max(map(len, a_seqs)), max(map(len, b_seqs))
	a, b = np.zeros((N, max(La, 1)), dtype = np.int32), np.zeros((N, max(Lb, 1)), dtype = np.int32)
	for i, (s, t) in enumerate(zip(a_seqs, b_seqs)):
		a[i, :len(s)], b[i, :len(t)] = s, t
	lengths = torch.from_numpy(np.array([[len(s) for s in a_seqs], [len(t) for t in b_seqs]], dtype = np.int32)).to(device)
	ai, bi, n, _ = nw_align(torch.from_numpy(a).to(device)[:, :La], lengths[0], torch.from_numpy(b).to(device)[:, :Lb], lengths[1], scores)
	host = torch.cat([n, ai.flatten(), bi.flatten()]).cpu().numpy()
	W = La + Lb
	n, ai, bi = host[:N], host[N:N + N * W].reshape(N, W), host[N + N * W:].reshape(N, W)
	return [(ai[p, :n[p]].tolist(), bi[p, :n[p]].tolist()) for p in range(N)]


def _aligned_units(index_a, index_b, a, b, unit_gap):
	"""The aligner's aligned sequences as the reference builds them: against a unit u the gap is placeholder * len(u) where the walk
	emitted it (unit_gap) and one placeholder in the leading / trailing runs that are emitted without walking."""
	n = len(index_a)
	gap_side = lambda k: 0 if index_a[k] < 0 else 1 if index_b[k] < 0 else None
	lead = 0  # a leading run of gaps on one side is the prefix: a walked gap is followed, further left, by a unit of that side
	while lead < n and gap_side(lead) is not None and gap_side(lead) == gap_side(0):
		lead += 1
	trail, tail_side = n, 0 if len(a) < len(b) else 1  # the tail pads the hypothesis when it is the shorter side, else the reference
	while trail > lead and gap_side(trail - 1) == tail_side:
		trail -= 1
	out_a, out_b = [], []
	for k, (i, j) in enumerate(zip(index_a, index_b)):
		walked = unit_gap and lead <= k < trail
		out_a.append(a[i] if i >= 0 else placeholder * (len(b[j]) if walked else 1))
		out_b.append(b[j] if j >= 0 else placeholder * (len(a[i]) if walked else 1))
	return out_a, out_b


def align_strings_batch(hyps, refs, aligner = None):
	"""align_strings over lists: [( _hyp_, _ref_ )] per pair.  Two aligner calls for the whole batch -- one over the word ids of every pair,
	one over the characters of every span of non-equal words of every pair -- so on the GPU two launches and two device-to-host copies,
	whatever the batch size (while the batch fits under ops.nw_align's workspace cap; a batch it has to split adds one launch per split;
	pairs past 16,383 units a side add one ops.nw_align_long call per level)."""
	aligner = aligner or gpu_aligner
	hyps, refs = list(hyps), list(refs)
	if len(hyps) != len(refs):
		raise ValueError(f'align_strings_batch: {len(hyps)} hypotheses for {len(refs)} references')
	hyp_words, ref_words = [h.split() for h in hyps], [r.split() for r in refs]
	ids = {}
	word_ids = lambda words: [[ids.setdefault(w, len(ids)) for w in ws] for ws in words]
	word_level = aligner(word_ids(hyp_words), word_ids(ref_words), WORD_ALIGN_SCORES)
	# per pair: pieces that are either an equal word (a string) or the number of a span to be aligned character by character
	pieces, span_hyp, span_ref = [], [], []
	for (index_a, index_b), hw, rw in zip(word_level, hyp_words, ref_words):
		cur, hyp_buffer, ref_buffer = [], [], []

		def flush():
			if hyp_buffer or ref_buffer:
				cur.append(len(span_hyp))
				span_hyp.append(space.join(hyp_buffer))
				span_ref.append(space.join(ref_buffer))
				hyp_buffer.clear()
				ref_buffer.clear()

		for h, r in zip(*_aligned_units(index_a, index_b, hw, rw, unit_gap = True)):
			if h == r:
				flush()
				cur.append(h)
			elif placeholder in h:
				ref_buffer.append(r)
			elif placeholder in r:
				hyp_buffer.append(h)
			else:
				ref_buffer.append(r)
				hyp_buffer.append(h)
		flush()
		pieces.append(cur)
	char_level = aligner([[ord(c) for c in s] for s in span_hyp], [[ord(c) for c in s] for s in span_ref], CHAR_ALIGN_SCORES)
	spans = [tuple(''.join(u) for u in _aligned_units(ia, ib, sh, sr, unit_gap = False)) for (ia, ib), sh, sr in zip(char_level, span_hyp, span_ref)]
	out = []
	for cur in pieces:
		_hyp_ = space.join(p if isinstance(p, str) else spans[p][0] for p in cur)
		_ref_ = space.join(p if isinstance(p, str) else spans[p][1] for p in cur)
		assert len(_hyp_) == len(_ref_)
		out.append((_hyp_, _ref_))
	return out


def align_strings(*, hyp, ref, aligner = None):
	"""metrics.align_strings (metrics.py:365-407): two strings of equal length, the hypothesis and the reference with placeholder '|' where
	the other side has a character the first lacks.  Two levels: (1) the word ids of hyp.split() / ref.split() are aligned (equal words,
	equal ids); (2) every maximal run of aligned words that are not equal is joined by spaces and aligned again character by character;
	(3) equal words and aligned runs are joined by spaces.  The aligned reference can gain spaces the input did not have
	(hyp 'б б', ref 'б' gives ('б б', 'б |')): the reference's behaviour, kept.

	Scores (match, sub, del, ins): (100, -6, -8, -3) for words and (5, -3, -4, -3) for characters.  These are what the reference RUNS
	with, not the tuples its signature shows ((100, -2, -8, -6) and (5, -2, -4, -3)): its unpacking assigns the fourth number to the
	substitution score and leaves the insertion score at the aligner's default -3.  A property of the reference, kept for parity.
	One departure: a word made only of two or more '|' characters is not told apart from a gap the way the reference would."""
	return align_strings_batch([hyp], [ref], aligner)[0]


def _split_word_pairs(_hyp_, _ref_, copy_space = False):
	"""Cuts a pair of aligned strings at the reference's spaces into (hyp word, ref word) pairs of equal length."""
	assert len(_hyp_) == len(_ref_)
	hyp, ref = list(_hyp_), list(_ref_)
	ref_chars = [i for i, c in enumerate(ref) if c != placeholder]
	first, last = (ref_chars[0], ref_chars[-1]) if ref_chars else (len(ref), -1)
	for i in range(len(ref)):  # the hypothesis' spaces outside the reference's extent become spaces of the reference
		if (i < first or i > last) and hyp[i] == space and ref[i] == placeholder:
			ref[i] = space
	if copy_space and ref_chars:  # a reference word glued to the start / the end of a longer hypothesis word is cut off it
		hyp_plain, ref_plain = replace_placeholder(''.join(hyp)), replace_placeholder(''.join(ref))
		if hyp_plain.endswith(ref_plain) and first - 1 >= 0 and hyp[first - 1] not in silence:
			ref[first - 1] = space
		if hyp_plain.startswith(ref_plain) and last + 1 < len(hyp) and hyp[last + 1] not in silence:
			ref[last + 1] = space
	ref.append(space)
	hyp.append(space)
	start, words = 0, []
	for i in range(len(ref)):
		if ref[i] != space:
			continue
		if hyp[i] in silence:
			stop, resume = i, i + 1
		else:  # the hypothesis runs on through this space: the space is undone; left of the reference's extent it stays with the word before it
			stop = resume = i + 1 if (ref_chars and i < first) else i
			ref[i] = placeholder
		if start != stop:
			words.append((''.join(hyp[start:stop]), ''.join(ref[start:stop])))
		start = resume
	return words


def _prefer_replacement(hyp, ref):
	"""An insertion next to a deletion becomes one replacement; columns that are gaps on both sides afterwards are dropped."""
	hyp, ref = list(hyp), list(ref)
	for k in range(len(ref) - 1):
		if ref[k] == placeholder and hyp[k] != placeholder and ref[k + 1] != placeholder and hyp[k + 1] == placeholder:
			ref[k], ref[k + 1] = ref[k + 1], placeholder
		elif hyp[k] == placeholder and ref[k] != placeholder and hyp[k + 1] != placeholder and ref[k + 1] == placeholder:
			hyp[k], hyp[k + 1] = hyp[k + 1], placeholder
	keep = [k for k in range(len(ref)) if not (hyp[k] == ref[k] == placeholder)]
	return ''.join(hyp[k] for k in keep), ''.join(ref[k] for k in keep)


class ErrorTagger:
	"""metrics.ErrorTagger (metrics.py:17-56): one tag per aligned word pair -- ok, typo_easy, typo_hard, missing, missing_ref."""
	typo_easy = 'typo_easy'
	typo_hard = 'typo_hard'
	missing = 'missing'
	missing_ref = 'missing_ref'
	ok = 'ok'

	error_tags = [typo_easy, typo_hard, missing, missing_ref]

	def tag(self, *, hyp, ref, hyp_tags = (), ref_tags = (), p = 0.5, L = 3, clamp = False):
		pairs = list(zip(hyp, ref))
		errors = sum(h != r for h, r in pairs if not (h == space and r == placeholder))
		errors_on_characters = sum(h != r for h, r in pairs if h not in silence and r not in silence)
		ok_except_end = all(h == r or k >= len(ref) - 2 or (h == space and r == placeholder) for k, (h, r) in enumerate(pairs))
		ref_gaps = ref.count(placeholder)
		ref_chars = len(ref) - ref_gaps
		hyp_empty, ref_empty = hyp.count(placeholder) == len(hyp), ref_gaps == len(ref)
		hyp_known = WordTagger.vocab_hit in hyp_tags or WordTagger.stop in hyp_tags
		vocab_typo_easy = (ref_empty and hyp_known) or (hyp_empty and WordTagger.stop in ref_tags)
		short_typo = len(ref) == 1 or (ref_chars == 0 and len(hyp) < L) or (0 < ref_chars < L and len(hyp) <= L)
		short_few_replacements = ref_chars < L and errors_on_characters <= 1
		is_typo = vocab_typo_easy or short_typo or (errors >= 0 and hyp.count(placeholder) < p * len(ref) and ref_gaps < p * len(ref))
		if hyp == ref:
			error_tag = self.ok
		elif is_typo:
			easy = vocab_typo_easy or short_few_replacements or errors <= 1 or (len(ref) > 2 and errors == 2 and ok_except_end) or (len(ref) >= 5 and errors <= 2)
			error_tag = self.typo_easy if easy else self.typo_hard
		else:
			error_tag = self.missing_ref if ref_gaps >= p * len(ref) else self.missing
		if clamp:
			errors = errors if error_tag in (self.typo_easy, self.ok) else -1 if error_tag == self.typo_hard else -2
		return error_tag, errors


class WordTagger(dict):
	"""metrics.WordTagger (metrics.py:59-76): vocab_hit / vocab_miss by membership in `vocab`, plus the tag of word_tags whose word list
	holds the word's stem (e.g. 'stop').  The default stemmer is the identity."""
	vocab_hit = 'vocab_hit'
	vocab_miss = 'vocab_miss'
	stop = 'stop'

	def __init__(self, stemmer = None, word_tags = {}, vocab = set()):
		super().__init__()
		self.stemmer = stemmer if stemmer is not None else (lambda word: word)
		self.vocab = vocab
		self.stem2tag = {self.stemmer(word): tag for tag, words in word_tags.items() for word in words}

	def __missing__(self, word):
		self[word] = self.stem2tag.get(self.stemmer(word))
		return self[word]

	def tag(self, word):
		word_tag = self[word]
		return [self.vocab_hit if word in self.vocab else self.vocab_miss] + ([word_tag] if word_tag else [])


def _word_alignment(_hyp_, _ref_, word_tagger, error_tagger, postproc):
	"""align_words without the per-word CER."""
	word_pairs = _split_word_pairs(_hyp_, _ref_)
	if postproc:
		word_pairs = [pair for hw, rw in word_pairs for pair in _split_word_pairs(*_prefer_replacement(hw, rw), copy_space = True)]
	words = []
	for hyp_word, ref_word in word_pairs:
		assert len(hyp_word) == len(ref_word)
		w = dict(_hyp_ = hyp_word, _ref_ = ref_word, hyp = replace_placeholder(hyp_word), ref = replace_placeholder(ref_word))
		w['ref_tags'] = word_tagger.tag(w['ref'])
		w['hyp_tags'] = word_tagger.tag(w['hyp'])
		w['error_tags'] = [error_tagger.tag(hyp = w['hyp'], ref = w['ref'], hyp_tags = w['hyp_tags'], ref_tags = w['ref_tags'])[0]]
		w['error_tag'] = w['error_tags'][0]
		w['len'] = len(w['ref'])
		words.append(w)
	return words


def _add_word_cer(alignments, scorer):
	"""w['cer'] for every word of every alignment, one scorer call."""
	words = [w for alignment in alignments for w in alignment]
	for w, c in zip(words, scorer([w['hyp'] for w in words], [w['ref'] for w in words])[0]):
		w['cer'] = c


def align_words(_hyp_, _ref_, word_tagger = None, error_tagger = None, postproc = False, compute_cer = False, scorer = None):
	"""metrics.align_words (metrics.py:261-362): the word pairs of a pair of aligned strings (align_strings' result), each a dict with
	_hyp_ / _ref_ (aligned), hyp / ref (placeholders removed), ref_tags / hyp_tags (word_tagger), error_tags / error_tag (error_tagger), len
	and, with compute_cer, cer (all words in one scorer call; default cer_wer on the GPU).  postproc: adjacent insertion + deletion become a
	replacement and a reference word glued to an end of a longer hypothesis word is cut off."""
	words = _word_alignment(_hyp_, _ref_, WordTagger() if word_tagger is None else word_tagger, error_tagger or ErrorTagger(), postproc)  # (an unused WordTagger is an empty dict: falsy)
	if compute_cer:
		_add_word_cer([words], scorer or cer_wer)
	return words


def extract_metric_value(analysis_result, key, sep = '.', missing = None):
	keys = key.split(sep)
	assert len(keys) <= 2
	value = analysis_result
	for k in keys:
		if not isinstance(value, dict):
			return missing
		value = value.get(k, missing)
	return value


def nanmean(list_of_dicts, key, sep = '.', missing = -1.0):
	"""metrics.nanmean (metrics.py:247-253): the mean of the finite values under `key`, summed in order; `missing` when there are none."""
	vals = [v for v in (extract_metric_value(d, key, sep) for d in list_of_dicts) if v is not None and math.isfinite(v)]
	return sum(vals) / len(vals) if vals else missing


class ErrorAnalyzer:
	"""metrics.ErrorAnalyzer (metrics.py:78-232).  configs: name -> dict of filter_words' keyword arguments (word_include_tags,
	word_exclude_tags, error_include_tags, error_exclude_tags) and optionally 'postprocessor', a key of `postprocessors`; empty configs mean
	dict(default = {}).  aligner / scorer: see the section comment; None = the GPU."""

	def __init__(self, word_tagger = None, error_tagger = None, configs = {}, postprocessors = {}, aligner = None, scorer = None):
		self.word_tagger = word_tagger if word_tagger is not None else WordTagger()
		self.error_tagger = error_tagger if error_tagger is not None else ErrorTagger()
		self.configs = configs or dict(default = {})
		self.postprocessors = postprocessors
		self.aligner = aligner
		self.scorer = scorer

	def aggregate(self, analyzed, sep = '__', defaults = {}):
		"""The validation line's numbers: nanmean of every numeric key of the analyses (config keys as config__key, the default config's
		also bare), and errors = dict(distribution: clamped error count -> words, words: the word pairs that are not ok)."""
		numeric = lambda d: [k for k, v in d.items() if isinstance(v, (float, int))]
		keys = numeric(analyzed[0])
		for c in self.configs:
			keys += [c + sep + k for k in numeric(analyzed[0].get(c, {}))]
		stats = dict(defaults)
		stats.update({k: nanmean(analyzed, k, sep = sep) for k in keys})
		prefix = 'default' + sep
		stats.update({name[len(prefix):]: value for name, value in list(stats.items()) if name.startswith(prefix)})
		distribution, error_words = collections.defaultdict(int), []
		for a in analyzed:
			for w in a.get('alignment', []):
				error_tag, errors = self.error_tagger.tag(hyp = w['hyp'], ref = w['ref'], clamp = True)
				distribution[errors] += 1
				if error_tag != ErrorTagger.ok:
					error_words.append(w)
		stats['errors'] = dict(distribution = dict(sorted(distribution.items())), words = error_words)
		return stats

	def filter_words(self, word_alignment, word_include_tags = [], word_exclude_tags = [], error_include_tags = [], error_exclude_tags = [], **kwargs):
		word_include_tags, word_exclude_tags, error_include_tags, error_exclude_tags = map(set, [word_include_tags, word_exclude_tags, error_include_tags, error_exclude_tags])
		res = []
		for w in word_alignment:
			ref_tags, error_tags = set(w['ref_tags']), set(w['error_tags'])
			if ref_tags & word_exclude_tags or error_tags & error_exclude_tags:
				continue
			if (word_include_tags and not ref_tags & word_include_tags) or (error_include_tags and not error_tags & error_include_tags):
				continue
			res.append(w)
		return res

	def compute_wordwise_metrics(self, filtered_alignment):
		n = len(filtered_alignment)
		n_ok = sum(ErrorTagger.ok in w['error_tags'] for w in filtered_alignment)
		n_missing = sum(ErrorTagger.missing in w['error_tags'] for w in filtered_alignment)
		return dict(
			num_words = n, num_words_ok = n_ok, num_words_missing = n_missing,
			mer_wordwise = n_missing / n if n != 0 else 0,
			wer_wordwise = 1.0 - n_ok / n if n != 0 else 0,
			cer_wordwise = sum(w['cer'] for w in filtered_alignment) / n if n != 0 else 0)

	def compute_vocabness_metrics(self, word_alignment, filtered_alignment, postprocess_transcript = None, **kwargs):
		n = len(filtered_alignment)
		hit = lambda k: sum(self.word_tagger.vocab_hit in w[k] for w in filtered_alignment) / n if n != 0 else 0
		return dict(ref_vocabness = hit('ref_tags'), hyp_vocabness = hit('hyp_tags'))

	@staticmethod
	def _corrected(word_alignment, filtered_alignment, postprocess_transcript, correct_filtered):
		"""(hyp, ref) texts in which the FILTERED words (correct_filtered) or all the OTHER words are replaced by the ground truth; a word
		counts as filtered when it equals a filtered one, as the reference's `w in filtered_alignment` does."""
		chosen = {(w['_hyp_'], w['_ref_']) for w in filtered_alignment}
		hyp = space.join(w['ref'] if ((w['_hyp_'], w['_ref_']) in chosen) == correct_filtered else w['hyp'] for w in word_alignment)
		return postprocess_transcript(hyp), postprocess_transcript(space.join(w['ref'] for w in word_alignment))

	def compute_pseudo_metrics(self, word_alignment, filtered_alignment, postprocess_transcript = None, **kwargs):
		"""What CER / WER would be if the filtered words were right."""
		c, w = (self.scorer or cer_wer)(*[[s] for s in self._corrected(word_alignment, filtered_alignment, postprocess_transcript or (lambda s: s), True)])
		return dict(cer_pseudo = c[0], wer_pseudo = w[0])

	def compute_filtered_metrics(self, word_alignment, filtered_alignment, postprocess_transcript = None, **kwargs):
		"""What CER / WER would be if all but the filtered words were right."""
		c, w = (self.scorer or cer_wer)(*[[s] for s in self._corrected(word_alignment, filtered_alignment, postprocess_transcript or (lambda s: s), False)])
		return dict(cer_filtered = c[0], wer_filtered = w[0])

	def analyze_batch(self, hyps, refs, postprocess_fn = None, detailed = False, extra = None, split_candidates = None):
		"""analyze over lists, with a constant number of aligner and scorer calls for the whole batch (on the GPU: two alignment launches
		and two launches per scorer call, of which there are at most four -- split candidates, the utterances, the words, the corrected
		texts of every config).  extra: one dict per utterance, or None."""
		hyps, refs = list(hyps), list(refs)
		if len(hyps) != len(refs):
			raise ValueError(f'analyze_batch: {len(hyps)} hypotheses for {len(refs)} references')
		scorer = self.scorer or cer_wer
		if split_candidates is not None:  # per utterance the (hyp, ref) candidate pair of least CER, ties by the strings
			cands = [[(h, r) for r in split_candidates(ref) for h in split_candidates(hyp)] for hyp, ref in zip(hyps, refs)]
			flat = [p for c in cands for p in c]
			cers = iter(scorer([h for h, r in flat], [r for h, r in flat])[0])
			chosen = [min((next(cers), p) for p in c)[1] for c in cands]
			hyps, refs = [h for h, r in chosen], [r for h, r in chosen]
		post = postprocess_fn if postprocess_fn is not None else (lambda s: s)
		post_hyps, post_refs = [post(h) for h in hyps], [post(r) for r in refs]
		cers, wers = scorer(post_hyps, post_refs)
		results = [dict(ref = pr, hyp = ph, ref_orig = r, hyp_orig = h, cer = c, wer = w, **(extra[k] if extra is not None else {}))
		           for k, (h, r, ph, pr, c, w) in enumerate(zip(hyps, refs, post_hyps, post_refs, cers, wers))]
		if not detailed:
			return results
		aligned = align_strings_batch(post_hyps, post_refs, self.aligner)
		alignments = [_word_alignment(_hyp_, _ref_, self.word_tagger, self.error_tagger, postproc = False) for _hyp_, _ref_ in aligned]
		_add_word_cer(alignments, scorer)
		corrected = []  # (result, config name, key stem, hyp text, ref text), scored in one call below
		for res, (_hyp_, _ref_), word_alignment in zip(results, aligned, alignments):
			res['alignment'] = word_alignment
			stats = dict(ok = 0, replace = 0, delete = 0, insert = 0, delete_spaces = 0, insert_spaces = 0, total_spaces = 0)
			for ch, cr in zip(_hyp_, _ref_):
				stats['ok'] += cr == ch
				stats['replace'] += cr != placeholder and cr != ch and ch != placeholder
				stats['delete'] += cr != placeholder and cr != ch and ch == placeholder
				stats['insert'] += cr == placeholder and ch != placeholder
				stats['delete_spaces'] += cr == space and ch != space
				stats['insert_spaces'] += ch == space and cr != space
				stats['total_spaces'] += cr == space
			res['char_stats'] = stats
			for name, config in self.configs.items():
				postprocess = self.postprocessors[config['postprocessor']] if 'postprocessor' in config else (lambda s: s)
				filtered = self.filter_words(word_alignment, **config)
				res[name] = self.compute_wordwise_metrics(filtered)
				corrected.append((res, name, 'filtered', *self._corrected(word_alignment, filtered, postprocess, False)))
				corrected.append((res, name, 'pseudo', *self._corrected(word_alignment, filtered, postprocess, True)))
		cers, wers = scorer([c[3] for c in corrected], [c[4] for c in corrected])
		for (res, name, stem, _, _), c, w in zip(corrected, cers, wers):
			res[name]['cer_' + stem], res[name]['wer_' + stem] = c, w
		for res in results:
			for name, config in self.configs.items():
				res[name].update(self.compute_vocabness_metrics(res['alignment'], self.filter_words(res['alignment'], **config)))
		return results

	def analyze(self, hyp, ref, postprocess_fn = None, detailed = False, extra = {}, split_candidates = None):
		"""metrics.ErrorAnalyzer.analyze (metrics.py:184-232) for one pair: the batch of one."""
		return self.analyze_batch([hyp], [ref], postprocess_fn = postprocess_fn, detailed = detailed, extra = [extra], split_candidates = split_candidates)[0]
