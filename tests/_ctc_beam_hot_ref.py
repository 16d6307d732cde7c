"""float64 restatement of the hot-phrase CTC prefix beam search that convasr_ctc_beam_search_hot / _lm_hot run on the GPU
(include/convasr_hip.h, the hot-phrase section).

It is the LM-free restatement (_ctc_beam_ref.py), or with a Model the LM one (_ctc_beam_lm_ref.py), plus the hot rule:
  state     every prefix has (m, k): m = the labels matched so far, a prefix of some phrase (() = the root), or None (DEAD); k = the labels
            matched since the last completed phrase.  The empty prefix has ((), 0).
  l + c     match: m is not None and m + (c,) is a prefix of a phrase: delta = +w, state (m + (c,), 0 if that is a phrase else k + 1)
            word start: otherwise, last(l) == s and (c,) is a prefix of a phrase: delta = -(w * k) + w, state ((c,), 0 if a phrase else 1)
            otherwise: delta = -(w * k), state ((), 0) if c == s else (None, 0)
  fusion    delta is added to every contribution to nnb(l + c), after the LM term: the extension's score and a fold into a held beam
  end       ranking score lpb + lpnb (+ F) + -(w * k); topk by it (ties: rank), and that is the returned score
Everything is derived from the prefix's labels: tuples of classes and sets of phrase prefixes, not the kernel's trie tables.

decode_one also returns min_gap (as the two restatements do, the final re-ranking included) and event counters: phrases completed, partial
matches revoked in mid-utterance, restarts at a word start, revocations at the end of the utterance (among the returned hypotheses) and
folds that carried a non-zero delta.  The first three are counted once per prefix the search creates."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ctc_beam_ref import pruned_classes  # noqa: E402
from _ctc_beam_lm_ref import OOV_SCORE  # noqa: E402

EVENTS = ('completed', 'revoked', 'restarts', 'end_revoked', 'folds')


class Hot:
	"""phrases: strings; labels: one character per class; weight: w."""

	def __init__(self, phrases, labels, weight):
		self.labels = list(str(labels).lower())
		self.C = len(self.labels)
		assert self.labels.count(' ') == 1
		self.space = self.labels.index(' ')
		first = {}
		for c, ch in enumerate(self.labels):
			first.setdefault(ch, c)
		self.w = float(weight)
		self.phrases = {tuple(first[ch] for ch in ' '.join(p.lower().split())) for p in phrases}
		assert all(p and p[0] != self.space and p[-1] != self.space for p in self.phrases)
		self.prefixes = {p[:k] for p in self.phrases for k in range(1, len(p) + 1)}
		self._rows = {}

	def step(self, state, last, c):
		"""(delta, new state, kind) of appending c to a prefix in `state` whose last label is `last`."""
		m, k = state
		w = self.w
		if m is not None and m + (c,) in self.prefixes:
			v = m + (c,)
			return w, (v, 0 if v in self.phrases else k + 1), 'match'
		if last == self.space and (c,) in self.prefixes:
			v = (c,)
			return -(w * k) + w, (v, 0 if v in self.phrases else 1), 'restart'
		return -(w * k), (() if c == self.space else None, 0), 'mismatch'

	def row(self, state, last):
		"""delta for every class (C,)."""
		key = (state, last == self.space)
		r = self._rows.get(key)
		if r is None:
			r = self._rows[key] = np.array([self.step(state, last, c)[0] for c in range(self.C)], dtype = np.float64)
		return r


def decode_one(lp, blank, H, W, N, cutoff_prob = 1.0, topk = 1, M = None):
	"""lp: (L, C) log-probabilities of one utterance; H: a Hot; M: None or a _ctc_beam_lm_ref.Model.  Returns (hyps, min_gap, events);
	hyps = [(tokens, offsets, ranking score)]."""
	lp = np.asarray(lp, dtype = np.float64)
	L = lp.shape[0] if lp.ndim == 2 else 0
	C = H.C
	space = H.space
	assert M is None or (M.space == space and M.blank == blank)
	NEG = -np.inf
	ev = dict.fromkeys(EVENTS, 0)
	every = np.ones(C, dtype = bool)
	every[blank] = False
	trie, trie_parent = {}, [-1]
	# per prefix id: (completed words, current word, allowed (C,), LM term of a space extension or None, hot state)
	pstate = [((), '', M.allowed('') if M is not None else every, None, ((), 0))]
	node_parent, node_token, node_frame = [], [], []
	pid, node, last = [0], [-1], [-1]
	lpb, lpnb = np.array([0.0]), np.array([NEG])
	min_gap = np.inf

	def child_state(p, c, plast):
		words, cw, allowed, sp, hs = pstate[p]
		if M is not None:
			if c == space:
				words, cw = words + (cw,), ''
			else:
				cw = cw + M.labels[c]
			allowed, sp = M.allowed(cw), (M.term(words, cw) if cw in M.vocab else None)
		_, ns, kind = H.step(hs, plast, c)
		if ns[0] in H.phrases:
			ev['completed'] += 1
		if kind != 'match' and hs[1] > 0:
			ev['revoked'] += 1
		if kind == 'restart':
			ev['restarts'] += 1
		return (words, cw, allowed, sp, ns)

	for t in range(L):
		P, margin = pruned_classes(lp[t], N, cutoff_prob)
		min_gap = min(min_gap, margin)
		n = len(pid)
		tot = np.logaddexp(lpb, lpnb)
		plp = lp[t, P]
		in_p = {int(c): k for k, c in enumerate(P)}
		last_a = np.array(last)
		allow = np.stack([pstate[p][2] for p in pid])[:, P] if n else np.zeros((0, len(P)), dtype = bool)
		delta = np.stack([H.row(pstate[p][4], l) for p, l in zip(pid, last)])[:, P] if n else np.zeros((0, len(P)))
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
		if M is not None and space in in_p:
			ext[:, in_p[space]] += np.array([pstate[p][3] if pstate[p][3] is not None else NEG for p in pid])
		ext = ext + delta
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
			if delta[i, k] != 0.0:
				ev['folds'] += 1
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
					pstate.append(child_state(pid[i], c, last[i]))
				node_parent.append(node[i]); node_token.append(c); node_frame.append(t)
				new_pid.append(kid); new_node.append(len(node_parent) - 1); new_last.append(c)
				new_lpb.append(NEG); new_lpnb.append(float(ext[i, src_k[e]]))
		pid, node, last = new_pid, new_node, new_last
		lpb, lpnb = np.array(new_lpb), np.array(new_lpnb)
	tot = np.logaddexp(lpb, lpnb)
	fin = np.empty(len(pid))
	for r, p in enumerate(pid):
		words, cw, _, sp, hs = pstate[p]
		f = tot[r]
		if M is not None:
			f = f + (0.0 if cw == '' else (sp if sp is not None else M.alpha * OOV_SCORE + M.beta))
		fin[r] = f + -(H.w * hs[1])
	rank = np.lexsort((np.arange(len(pid)), -fin))
	hyps = []
	for r in rank[:topk]:
		toks, offs = [], []
		k = node[r]
		while k >= 0:
			toks.append(node_token[k]); offs.append(node_frame[k])
			k = node_parent[k]
		hyps.append((toks[::-1], offs[::-1], float(fin[r])))
		if pstate[pid[r]][4][1] > 0:
			ev['end_revoked'] += 1
	for a, b in zip(rank[:topk], rank[1:topk + 1]):
		min_gap = min(min_gap, float(fin[a] - fin[b]))
	return hyps, min_gap, ev


def decode(log_probs_btc, lengths, blank, H, W, N, cutoff_prob = 1.0, topk = 1, M = None):
	"""Batch form in the layout of convasr_ctc_beam_search_hot (log_prob float64): (tokens, offsets, out_lengths, log_prob, min_gap, events)."""
	lp = np.asarray(log_probs_btc, dtype = np.float64)
	B, T, C = lp.shape
	tokens = np.zeros((B, topk, T), dtype = np.int64)
	offsets = np.zeros((B, topk, T), dtype = np.int32)
	out_len = np.zeros((B, topk), dtype = np.int64)
	logp = np.full((B, topk), -np.inf)
	min_gap = np.inf
	events = dict.fromkeys(EVENTS, 0)
	for b in range(B):
		hyps, gap, ev = decode_one(lp[b, :int(lengths[b])], blank, H, W, N, cutoff_prob, topk, M)
		min_gap = min(min_gap, gap)
		for k in EVENTS:
			events[k] += ev[k]
		for k, (toks, offs, s) in enumerate(hyps):
			tokens[b, k, :len(toks)] = toks
			offsets[b, k, :len(offs)] = offs
			out_len[b, k] = len(toks)
			logp[b, k] = s
	return tokens, offsets, out_len, logp, min_gap, events
