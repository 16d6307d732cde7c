"""float64 restatement of the LM-fused CTC prefix beam search that convasr_ctc_beam_search_lm runs on the GPU (include/convasr_hip.h).

It is the LM-free restatement (_ctc_beam_ref.py) with the rules of the header's LM section:
  labels    one character per class, lowercased; the space class s is the one labelled ' '
  V         the unigrams other than <s>, </s>, <unk> whose characters all map to classes other than the blank and s
  LM term   lm(w | words) = alpha * ln P(w | ctx) + beta, ln = log10 * ln 10; ctx = the last N_lm - 1 completed words, <s> in front of fewer;
            log10 P by the backoff rule over the full context (a context that is not listed has backoff weight 0)
  cw(l)     the characters after the last space of l
  allowed   l + c for c not blank / s (extension, not the stay of a repeated last token): cw(l) + labels[c] is a prefix of a word in V;
            l + s: cw(l) non-empty and in V
  fusion    every contribution to nnb(l + s) (from lpb(l), lpnb(l), and a fold into a held beam) gets lm(cw(l) | words(l)) added
  end       ranking score lpb + lpnb + F(l): F = 0 for an empty l or one ending in s, lm(cw(l)) when cw(l) in V, alpha * -1000 + beta
            otherwise; topk by it (ties: rank), and that is the returned score.
  no beams  when a frame leaves no candidate (no allowed class and no blank among P_t), the search has no hypothesis left: every slot of
            the utterance gets length 0 and -inf.
This module derives everything from the prefix's labels directly (words split at s, a set of word prefixes, a dict of n-grams), not
from the kernel's trie / state tables."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ctc_beam_ref import pruned_classes  # noqa: E402

SPECIAL = ('<s>', '</s>', '<unk>')
OOV_SCORE = -1000.0
LN10 = math.log(10.0)


def log10_cond(ngrams, order, words, w):
	"""log10 P(w | words) by the backoff rule: context = the last order - 1 words, <s> in front when there are fewer."""
	if order == 1:
		h = ()
	else:
		h = tuple(words)
		h = (('<s>',) + h)[-(order - 1):] if len(h) < order - 1 else h[-(order - 1):]
	acc = 0.0
	for j in range(len(h) + 1):
		g = h[j:]
		hit = ngrams.get(g + (w,))
		if hit is not None:
			return acc + hit[0]
		if g:
			acc += ngrams.get(g, (0.0, 0.0))[1]
	raise KeyError(w)


class Model:
	"""The LM as the restatement uses it: arpa (order, ngrams, words), labels (a string), blank, alpha, beta."""

	def __init__(self, arpa, labels, blank, alpha, beta):
		self.labels = list(str(labels).lower())
		self.C = len(self.labels)
		assert self.labels.count(' ') == 1
		self.space = self.labels.index(' ')
		assert self.space != blank
		self.blank, self.alpha, self.beta = blank, float(alpha), float(beta)
		self.order, self.ngrams = arpa.order, arpa.ngrams
		first = {}
		for c, ch in enumerate(self.labels):
			first.setdefault(ch, c)
		ok = lambda w: w not in SPECIAL and all(first.get(ch, -1) >= 0 and first[ch] not in (blank, self.space) for ch in w)
		self.vocab = {w for w in arpa.words if w and ok(w)}
		self.prefixes = {w[:k] for w in self.vocab for k in range(1, len(w) + 1)}
		self._allowed = {}

	def term(self, words, w):
		return self.alpha * (log10_cond(self.ngrams, self.order, words, w) * LN10) + self.beta

	def allowed(self, cw):
		"""Bool (C,): the classes c for which l + c may be created from a prefix whose current word is cw (blank: False)."""
		a = self._allowed.get(cw)
		if a is None:
			a = np.array([c != self.blank and (cw != '' and cw in self.vocab if c == self.space else (cw + self.labels[c]) in self.prefixes)
			              for c in range(self.C)])
			self._allowed[cw] = a
		return a


def decode_one(lp, M, W, N, cutoff_prob = 1.0, topk = 1):
	"""lp: (L, C) log-probabilities of one utterance; M: a Model.  Returns (hyps, min_gap); hyps = [(tokens, offsets, fused score)]."""
	lp = np.asarray(lp, dtype = np.float64)
	L = lp.shape[0] if lp.ndim == 2 else 0
	blank, space = M.blank, M.space
	NEG = -np.inf
	trie, trie_parent = {}, [-1]
	# per prefix id: (completed words, current word, allowed (C,), LM term of a space extension or None)
	pstate = [((), '', M.allowed(''), None)]
	node_parent, node_token, node_frame = [], [], []
	pid, node, last = [0], [-1], [-1]
	lpb, lpnb = np.array([0.0]), np.array([NEG])
	min_gap = np.inf

	def child_state(p, c):
		words, cw, _, sp = pstate[p]
		if c == space:
			words, cw = words + (cw,), ''
		else:
			cw = cw + M.labels[c]
		return (words, cw, M.allowed(cw), M.term(words, cw) if cw in M.vocab else None)

	for t in range(L):
		P, margin = pruned_classes(lp[t], N, cutoff_prob)
		min_gap = min(min_gap, margin)
		n = len(pid)
		tot = np.logaddexp(lpb, lpnb)
		plp = lp[t, P]
		in_p = {int(c): k for k, c in enumerate(P)}
		last_a = np.array(last)
		lmsp = np.array([pstate[p][3] if pstate[p][3] is not None else NEG for p in pid])
		allow = np.stack([pstate[p][2] for p in pid])[:, P] if n else np.zeros((0, len(P)), dtype = bool)  # (every beam may die: see the header)
		nb = np.full(n, NEG)
		nnb = np.full(n, NEG)
		got = np.zeros(n, dtype = bool)
		if blank in in_p:
			nb = plp[in_p[blank]] + tot
			got[:] = True
		for i in range(n):
			if last[i] >= 0 and last[i] in in_p:
				nnb[i] = plp[in_p[last[i]]] + lpnb[i]
				got[i] = True
		ext = plp[None, :] + np.where(P[None, :] == last_a[:, None], lpb[:, None], tot[:, None])
		if space in in_p:
			ext[:, in_p[space]] += lmsp
		ext_ok = allow & (P[None, :] != blank)
		where = {p: i for i, p in enumerate(pid)}
		for j in range(n):
			if last[j] < 0 or last[j] not in in_p:
				continue
			i = where.get(trie_parent[pid[j]])
			if i is None:
				continue
			k = in_p[last[j]]
			if not allow[i, k]:
				continue
			nnb[j] = np.logaddexp(nnb[j], ext[i, k])
			got[j] = True
			ext_ok[i, k] = False
		own = np.logaddexp(nb, nnb)
		own_ok = got & (own > NEG)
		ext_ok &= ext > NEG
		ii, kk = np.nonzero(ext_ok)
		oi = np.nonzero(own_ok)[0]
		score = np.concatenate([own[oi], ext[ii, kk]])
		key_r = np.concatenate([oi, ii])
		key_c = np.concatenate([np.full(len(oi), -1), P[kk]])
		src_own = np.concatenate([np.ones(len(oi), dtype = bool), np.zeros(len(ii), dtype = bool)])
		src_k = np.concatenate([np.zeros(len(oi), dtype = np.int64), kk])
		m = len(score)
		if m > W:
			v = -np.partition(-score, W - 1)[W - 1]
			sub = np.nonzero(score >= v)[0]
		else:
			sub = np.arange(m)
		order = sub[np.lexsort((key_c[sub], key_r[sub], -score[sub]))]
		if m > W:
			rest = np.delete(score, order[:W])
			min_gap = min(min_gap, float(score[order[W - 1]] - rest.max()))
		order = order[:W]
		new_pid, new_node, new_last, new_lpb, new_lpnb = [], [], [], [], []
		for e in order:
			i = int(key_r[e])
			if src_own[e]:
				new_pid.append(pid[i]); new_node.append(node[i]); new_last.append(last[i])
				new_lpb.append(nb[i]); new_lpnb.append(nnb[i])
			else:
				c = int(key_c[e])
				kid = trie.get((pid[i], c))
				if kid is None:
					kid = trie[(pid[i], c)] = len(trie_parent)
					trie_parent.append(pid[i])
					pstate.append(child_state(pid[i], c))
				node_parent.append(node[i]); node_token.append(c); node_frame.append(t)
				new_pid.append(kid); new_node.append(len(node_parent) - 1); new_last.append(c)
				new_lpb.append(NEG); new_lpnb.append(float(ext[i, src_k[e]]))
		pid, node, last = new_pid, new_node, new_last
		lpb, lpnb = np.array(new_lpb), np.array(new_lpnb)
	tot = np.logaddexp(lpb, lpnb)
	oov = M.alpha * OOV_SCORE + M.beta
	fin = np.empty(len(pid))
	for r, p in enumerate(pid):
		words, cw, _, sp = pstate[p]
		fin[r] = tot[r] + (0.0 if cw == '' else (sp if sp is not None else oov))
	rank = np.lexsort((np.arange(len(pid)), -fin))
	hyps = []
	for r in rank[:topk]:
		toks, offs = [], []
		k = node[r]
		while k >= 0:
			toks.append(node_token[k]); offs.append(node_frame[k])
			k = node_parent[k]
		hyps.append((toks[::-1], offs[::-1], float(fin[r])))
	for a, b in zip(rank[:topk], rank[1:topk + 1]):
		min_gap = min(min_gap, float(fin[a] - fin[b]))
	return hyps, min_gap


def decode(log_probs_btc, lengths, M, W, N, cutoff_prob = 1.0, topk = 1):
	"""Batch form in the layout of convasr_ctc_beam_search_lm (log_prob float64)."""
	lp = np.asarray(log_probs_btc, dtype = np.float64)
	B, T, C = lp.shape
	tokens = np.zeros((B, topk, T), dtype = np.int64)
	offsets = np.zeros((B, topk, T), dtype = np.int32)
	out_len = np.zeros((B, topk), dtype = np.int64)
	logp = np.full((B, topk), -np.inf)
	min_gap = np.inf
	for b in range(B):
		hyps, gap = decode_one(lp[b, :int(lengths[b])], M, W, N, cutoff_prob, topk)
		min_gap = min(min_gap, gap)
		for k, (toks, offs, s) in enumerate(hyps):
			tokens[b, k, :len(toks)] = toks
			offsets[b, k, :len(offs)] = offs
			out_len[b, k] = len(toks)
			logp[b, k] = s
	return tokens, offsets, out_len, logp, min_gap


def lm_terms(M, labels_seq):
	"""The LM terms a labelling (class list) collects: one per space token (the word before it) plus F at the end."""
	words, cw, total = (), '', 0.0
	for c in labels_seq:
		if c == M.space:
			total += M.term(words, cw)
			words, cw = words + (cw,), ''
		else:
			cw += M.labels[c]
	if cw:
		total += M.term(words, cw) if cw in M.vocab else M.alpha * OOV_SCORE + M.beta
	return total


def is_allowed(M, labels_seq):
	"""Whether the dictionary constraint lets a labelling be produced (every step of it an allowed extension)."""
	cw = ''
	for c in labels_seq:
		if c == M.blank or not M.allowed(cw)[c]:
			return False
		cw = '' if c == M.space else cw + M.labels[c]
	return True
