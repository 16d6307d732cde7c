"""A numpy restatement of convasr_ctc_greedy_segments' rule (include/convasr_hip.h): every frame decides from its class, the class of the
previous non-blank frame and the blanks between them whether it emits.  tests/test_greedy_ref.py holds it against the host loop
(GreedyCTCGenerator.generate_host), tests/test_greedy_segments_gpu.py holds the kernel against it."""
import numpy as np


def greedy_segments(path, length, eps, space, bats, split_words = True):
	"""One utterance.  Returns (tokens, frames, segments): the emitted tokens, the frame of each, and per segment (index of its first token,
	begin frame, end frame)."""
	path = np.asarray(path, dtype = np.int64)
	T = len(path)
	n = min(max(int(length), 0), T)
	t = np.arange(T)
	speech = np.flatnonzero((t < n) & (path != eps) & (path != space))
	if len(speech) == 0:
		return [], [], []
	start = speech[0]
	active = (t >= start) & (t < n)
	nonblank = active & (path != eps)
	prev = np.maximum.accumulate(np.where(nonblank, t, -1))  # the last non-blank frame up to and including t
	prev = np.concatenate([[-1], prev[:-1]])  # ... before t
	prev_cls = np.where(prev >= 0, path[np.maximum(prev, 0)], eps)
	g = t - prev - 1
	emits = nonblank & ((t == start) | np.where(prev_cls == space, path != space, (g >= 1) | (path != prev_cls)))
	inserts = active & (path == eps) & (prev >= 0) & (prev_cls != space) & (t - prev == max(bats, 1))
	tokens, frames, segments = [], [], []
	for f in np.flatnonzero(emits | inserts):
		f = int(f)
		if inserts[f]:
			tokens.append(space)
			frames.append(f)
			continue
		c = int(path[f])
		if f == start or (split_words and c == space):
			segments.append([len(tokens), f, f])
			if f != start:
				tokens.append(c)
				frames.append(f)
		tokens.append(c)
		frames.append(f)
		segments[-1][2] = f
	return tokens, frames, [tuple(s) for s in segments]


def greedy_segments_batch(path, lengths, eps, space, bats, split_words = True):
	"""The packed outputs of ops.ctc_greedy_segments: (tokens, frames, counts (2, B), seg_first, seg_begin, seg_end) as lists."""
	tokens, frames, counts, first, begin, end = [], [], [[], []], [], [], []
	for b in range(len(path)):
		tk, fr, sg = greedy_segments(path[b], lengths[b], eps, space, bats, split_words)
		first += [len(tokens) + s[0] for s in sg]
		begin += [s[1] for s in sg]
		end += [s[2] for s in sg]
		tokens += tk
		frames += fr
		counts[0].append(len(tk))
		counts[1].append(len(sg))
	return tokens, frames, counts, first, begin, end


def segment_dicts(tokenizer, tokens, segments, begin, end, ts, key = 'hyp'):
	"""What GreedyCTCGenerator builds of one utterance's restated segments; ts: the utterance's time stamps as Python floats, or None."""
	out = []
	for k, (first, fb, fe) in enumerate(segments):
		last = segments[k + 1][0] if k + 1 < len(segments) else len(tokens)
		text = tokenizer.decode([tokens[first:last]])[0]
		out.append({'begin': begin + ts[fb], 'end': begin + ts[fe], key: text} if ts is not None else {'begin': begin, 'end': end, key: text})
	return out
