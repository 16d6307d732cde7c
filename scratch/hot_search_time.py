"""Timing of the hot-phrase CTC beam search on the GPU (README row, profiles/r18_hot_phrases.json).

The README's decode shape: 64 x 750 frames x 38 classes (seeded speech-like log-probs, scratch/keyword_search_time.py's), cutoff_top_n 40,
top 4, beam widths 64 and 1024.  By DEVICE EVENTS around the C entry points, buffers and tables allocated and uploaded outside, all in ONE
process and alternating, medians of 7 after 2 warm-ups with min and max:
  this tree's library   convasr_ctc_beam_search, _lm, _hot, _lm_hot (100 phrases of about 12 labels made of the LM's words, weight 1.0)
  --parent-lib PATH     the same two hot-less entry points of a library built from the parent commit, loaded beside it with ctypes
The margin a slowdown of the hot-less kernels gets is the parent's own min-max spread over its 7 runs; the file states both.
The LM is tests/_lm_synth.py's order-4 model of 10^5 words.  Usage: python scratch/hot_search_time.py [--parent-lib PATH] --out FILE"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lm_synth  # noqa: E402
from convasr_amd import _lib, hotwords, lm, ops  # noqa: E402
from convasr_amd.transcribe import RU_ALPHABET  # noqa: E402
from convasr_amd.transcript_generators import CharTokenizerLegacy  # noqa: E402
from greedy_segments_time import stats  # noqa: E402
from keyword_search_time import events, log_probs_like  # noqa: E402

B, T, N, TOPK, WEIGHT = 64, 750, 40, 4, 1.0
ALPHA, BETA = 0.4, 2.6


def phrases_of(model, blank, count, labels, seed):
	"""`count` phrases of about `labels` labels: words of the LM's vocabulary joined by spaces."""
	rng = np.random.RandomState(seed)
	words = sorted(model.vocabulary_of(blank))
	out = set()
	while len(out) < count:
		p = words[rng.randint(len(words))]
		while len(p) < labels - 3:
			p += ' ' + words[rng.randint(len(words))]
		if len(p) <= labels + 3:
			out.add(p)
	return sorted(out)


def main(out, parent_path):
	d = torch.device('cuda:0')
	tok = CharTokenizerLegacy(RU_ALPHABET)
	C, blank = tok.vocab_size, tok.eps_id
	labels = ''.join(tok.vocab)
	model = lm.NgramLM(_lm_synth.write(os.path.join(tempfile.mkdtemp(), 'big.arpa')), labels)
	phrases = phrases_of(model, blank, 100, 12, 7)
	hot = hotwords.HotWords(phrases, labels)
	hot.check_vocabulary(model, blank)
	lp, _ = log_probs_like(B, T, tok, d)
	lens = torch.full((B,), T, dtype = torch.int64, device = d)
	t, h = model.device_tables(blank, d), hot.device_tables(blank, d)
	P, S = _lib.ptr, _lib.stream_ptr
	tokens, offsets = torch.empty(B, TOPK, T, dtype = torch.int64, device = d), torch.empty(B, TOPK, T, dtype = torch.int32, device = d)
	out_len, logp = torch.empty(B, TOPK, dtype = torch.int64, device = d), torch.empty(B, TOPK, dtype = torch.float64, device = d)
	lm_args = (P(t['node_mask']), P(t['node_child']), P(t['node_word']), int(t['node_word'].numel()), P(t['ent_pb']), P(t['ent_sl']), int(t['ent_sl'].shape[0]), P(t['slots']),
	           int(t['slots'].shape[0]), model.space, model.order, model.start_state, ALPHA, BETA)
	hot_args = (P(h['hot_mask']), P(h['hot_child']), P(h['hot_term']), hot.num_nodes, int(h['hot_mask'].shape[1]))
	parent = None
	if parent_path:
		parent = ctypes.CDLL(os.path.abspath(parent_path))
		for name in ('convasr_ctc_beam_search', 'convasr_ctc_beam_search_lm', 'convasr_ctc_beam_search_lm_workspace_bytes'):
			getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGNATURES[name]
	lib = _lib.load()
	res = dict(device = torch.cuda.get_device_name(0), B = B, T = T, classes = C, cutoff_top_n = N, topk = TOPK, phrases = len(phrases), hot_trie_nodes = hot.num_nodes,
	           mean_phrase_labels = float(np.mean([len(p) for p in phrases])), weight = WEIGHT, lm = 'tests/_lm_synth.py order 4, 10^5 words', alpha = ALPHA, beta = BETA,
	           which_clock = 'DEVICE EVENTS around the C entry points, one MI355X, one process, alternating, medians of 7 after 2 warm-ups with min and max',
	           note = 'the log-probs are random speech-like frames, so a phrase is seldom spelled to its end; every frame still tests the masks and adds the delta for every candidate',
	           parent_library = bool(parent), widths = [])
	for W in (64, 1024):
		assert lib.convasr_ctc_beam_search_lm_hot_workspace_bytes(B, T, C, W, 38, TOPK) > 0  # the LDS forms
		ws = torch.empty(B * T * W * 8, dtype = torch.uint8, device = d)
		head = (P(lp), P(lens), P(tokens), P(offsets), P(out_len), P(logp), P(ws), B, T, C, blank, W, 38, 1.0, TOPK)
		fns = dict(beam_search = lambda: _lib.call('convasr_ctc_beam_search', *head, S()),
		           beam_search_lm = lambda: _lib.call('convasr_ctc_beam_search_lm', *head, *lm_args, S()),
		           beam_search_hot = lambda: _lib.call('convasr_ctc_beam_search_hot', *head, *hot_args, hot.space, WEIGHT, S()),
		           beam_search_lm_hot = lambda: _lib.call('convasr_ctc_beam_search_lm_hot', *head, *lm_args, *hot_args, WEIGHT, S()))
		if parent is not None:
			def checked(name, *a):
				assert getattr(parent, name)(*a) == 0, name
			fns['parent_beam_search'] = lambda: checked('convasr_ctc_beam_search', *head, S())
			fns['parent_beam_search_lm'] = lambda: checked('convasr_ctc_beam_search_lm', *head, *lm_args, S())
		times = events(fns)
		row = dict(W = W, device_events_ms = {k: stats(v) for k, v in times.items()})
		med = {k: statistics.median(v) for k, v in times.items()}
		row['hot_over_hotless'] = dict(no_lm = med['beam_search_hot'] / med['beam_search'], lm = med['beam_search_lm_hot'] / med['beam_search_lm'])
		if parent is not None:
			row['hotless_vs_parent'] = {k: dict(this_over_parent = med[k] / med['parent_' + k], parent_spread_over_median = (max(times['parent_' + k]) - min(times['parent_' + k])) / med['parent_' + k],
			                                    within_parent_spread = bool(med[k] - med['parent_' + k] <= max(times['parent_' + k]) - min(times['parent_' + k])))
			                            for k in ('beam_search', 'beam_search_lm')}
		res['widths'].append(row)
		print(json.dumps(row), flush = True)
		json.dump(res, open(out, 'w'), indent = 1)


if __name__ == '__main__':
	ap = argparse.ArgumentParser()
	ap.add_argument('--parent-lib', default = None)
	ap.add_argument('--out', default = os.path.join(ROOT, 'profiles', 'r18_hot_phrases.json'))
	a = ap.parse_args()
	assert torch.cuda.is_available(), 'this script measures on the GPU'
	main(a.out, a.parent_lib)
