"""float64 restatement of the CTC prefix beam search that convasr_ctc_beam_search runs on the GPU (include/convasr_hip.h).

Beam state: a prefix (collapsed label sequence) with lpb / lpnb = log-probability that it ends in blank / in a non-blank.
Per frame t:
  P_t      the classes sorted by lp[t] descending (ties: lower index first), the first N; with cutoff_prob < 1 only the shortest
           leading run whose cumulative probability reaches cutoff_prob (at least one class).  Blank is pruned like any other class.
  extend   for every beam l and c in P_t (`+` = logaddexp):
             c == blank:      nb(l)    += lp + (lpb + lpnb)(l)
             c == last(l):    nnb(l)   += lp + lpnb(l);  nnb(l + c) += lp + lpb(l)
             otherwise:       nnb(l+c) += lp + (lpb + lpnb)(l)
           an extension l_i + c equal to a beam l_j already held is folded into l_j's own candidate; a candidate that received no
           contribution, or whose total is -inf (probability zero), is dropped.
  select   the top W candidates by lpb + lpnb; ties by ascending key (rank of the source beam, -1) for a beam's own candidate,
           (rank of i, c) for an unmerged extension of beam i by c.  The same order is the next frame's ranking.
Offsets: a token's offset is the frame at which the extension that created its node appended it (folding keeps the existing node).

decode() returns per utterance the best topk beams (tokens, offsets, log-probability) and `min_gap`: the smallest score margin any
decision of the search rested on -- the gap between the W-th and (W+1)-th candidate of every frame, the gaps between consecutive
returned hypotheses, and (cutoff_prob < 1) the probability margin of every cut.  An implementation whose arithmetic differs from
this one by less than min_gap makes the same decisions."""
import numpy as np


def pruned_classes(lp_t, N, cutoff_prob):
	"""P_t: class indices (best first) and the probability margin of the cutoff (inf when no cut was made)."""
	order = np.argsort(-lp_t, kind = 'stable')[:N]
	margin = np.inf
	if cutoff_prob < 1.0:
		cum = np.cumsum(np.exp(lp_t[order].astype(np.float64)))
		hit = np.nonzero(cum >= cutoff_prob)[0]
		n = int(hit[0]) + 1 if len(hit) else len(order)
		n = max(n, 1)
		near = np.abs(cum - cutoff_prob)
		margin = float(near.min()) if len(near) else np.inf
		order = order[:n]
	return order, margin


def decode_one(lp, blank, W, N, cutoff_prob = 1.0, topk = 1):
	"""lp: (L, C) log-probabilities of one utterance (its valid frames).  Returns (hyps, min_gap); hyps = [(tokens, offsets, logp)]."""
	lp = np.asarray(lp, dtype = np.float64)
	L, C = lp.shape if lp.ndim == 2 else (0, 0)
	NEG = -np.inf
	trie, trie_parent = {}, [-1]  # prefix id -> (parent prefix id, token) is hash-consed: equal prefixes have equal ids
	node_parent, node_token, node_frame = [], [], []
	# beams in rank order: prefix id, node id, last token, lpb, lpnb
	pid, node, last = [0], [-1], [-1]
	lpb, lpnb = np.array([0.0]), np.array([NEG])
	min_gap = np.inf
	for t in range(L):
		P, margin = pruned_classes(lp[t], N, cutoff_prob)
		min_gap = min(min_gap, margin)
		n = len(pid)
		tot = np.logaddexp(lpb, lpnb)
		plp = lp[t, P]
		in_p = {int(c): k for k, c in enumerate(P)}
		last_a = np.array(last)
		# own candidates
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
		# extensions
		ext = plp[None, :] + np.where(P[None, :] == last_a[:, None], lpb[:, None], tot[:, None])
		ext_ok = np.broadcast_to(P[None, :] != blank, ext.shape).copy()
		where = {p: i for i, p in enumerate(pid)}
		for j in range(n):  # fold l_i + c == l_j into l_j
			if last[j] < 0 or last[j] not in in_p:
				continue
			i = where.get(trie_parent[pid[j]])
			if i is None:
				continue
			k = in_p[last[j]]
			nnb[j] = np.logaddexp(nnb[j], ext[i, k])
			got[j] = True
			ext_ok[i, k] = False
		own = np.logaddexp(nb, nnb)
		own_ok = got & (own > NEG)
		ext_ok &= ext > NEG
		# candidates: score, key = (rank, c) with c = -1 for own
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
				node_parent.append(node[i]); node_token.append(c); node_frame.append(t)
				new_pid.append(kid); new_node.append(len(node_parent) - 1); new_last.append(c)
				new_lpb.append(NEG); new_lpnb.append(float(ext[i, src_k[e]]))
		pid, node, last = new_pid, new_node, new_last
		lpb, lpnb = np.array(new_lpb), np.array(new_lpnb)
	tot = np.logaddexp(lpb, lpnb)
	hyps = []
	for r in range(min(topk, len(pid))):
		toks, offs = [], []
		k = node[r]
		while k >= 0:
			toks.append(node_token[k]); offs.append(node_frame[k])
			k = node_parent[k]
		hyps.append((toks[::-1], offs[::-1], float(tot[r])))
	for r in range(min(topk, len(pid) - 1)):
		min_gap = min(min_gap, float(tot[r] - tot[r + 1]))
	return hyps, min_gap


def decode(log_probs_btc, lengths, blank, W, N, cutoff_prob = 1.0, topk = 1):
	"""Batch form: log_probs (B, T, C), lengths (B,).  Returns (tokens (B, topk, T) int64, offsets (B, topk, T) int32,
	out_lengths (B, topk) int64, log_prob (B, topk) float64, min_gap) in the layout of convasr_ctc_beam_search: hypotheses past the
	last one a search produced have length 0 and log-probability -inf, positions past a hypothesis' length hold 0."""
	lp = np.asarray(log_probs_btc, dtype = np.float64)
	B, T, C = lp.shape
	tokens = np.zeros((B, topk, T), dtype = np.int64)
	offsets = np.zeros((B, topk, T), dtype = np.int32)
	out_len = np.zeros((B, topk), dtype = np.int64)
	logp = np.full((B, topk), -np.inf)
	min_gap = np.inf
	for b in range(B):
		hyps, gap = decode_one(lp[b, :int(lengths[b])], blank, W, N, cutoff_prob, topk)
		min_gap = min(min_gap, gap)
		for k, (toks, offs, s) in enumerate(hyps):
			tokens[b, k, :len(toks)] = toks
			offsets[b, k, :len(offs)] = offs
			out_len[b, k] = len(toks)
			logp[b, k] = s
	return tokens, offsets, out_len, logp, min_gap


def labelling_log_prob(lp, labels, blank):
	"""Exhaustive sum over every CTC path of length L that collapses to `labels` (brute force; tiny L only)."""
	import itertools
	lp = np.asarray(lp, dtype = np.float64)
	L, C = lp.shape
	total = -np.inf
	for path in itertools.product(range(C), repeat = L):
		out, prev = [], None
		for c in path:
			if c != blank and c != prev:
				out.append(c)
			prev = c
		if out == list(labels):
			total = np.logaddexp(total, sum(lp[t, c] for t, c in enumerate(path)))
	return total
