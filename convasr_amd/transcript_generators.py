"""Greedy CTC decoding (reference: transcript_generators.py:8-93, text_tokenizers.py:7-51).

The per-frame argmax over classes runs on the GPU (convasr_argmax).  The collapse rules -- skip leading blank/space, merge repeats
unless a blank intervened, >= blank_amount_to_space consecutive blanks insert one space, a blank right after a space is ignored, a new
segment starts at every word-start token when time stamps are given -- are GreedyCTCGenerator.generate_host, a host loop over B x t
ints as in the reference, and the oracle of everything else.  For CUDA log-probs and a tokenizer of CharTokenizerLegacy's kind
(silence = {eps, space}, word start = space) GreedyCTCGenerator.generate runs the same rules on the device instead
(ops.ctc_greedy_segments: tokens, their frames and the word segments, include/convasr_hip.h has the rule), gathers the time stamps at
the segments' begin / end frames there and copies only counts, tokens and those stamps: host work and device-to-host bytes grow with
the transcript, not with B x t.  CPU tensors, other tokenizers and output_lengths given as a list keep the host loop."""
import types

import torch

from . import ops
from ._lib import ConvasrHipError

UNCERTAINTY_KEYS = ('confidence', 'confidence_min', 'margin', 'entropy', 'uncertainty')  # what generate(..., uncertainty = True) adds to every Segment (ops.span_uncertainty)


class Segment(dict):
	pass


class Transcript(list):
	pass


class CharTokenizerLegacy:
	"""text_tokenizers.py:7-51: alphabet + ['*', '.', '2', ' ', '|']; eps ('|') is the CTC blank and the last class."""

	def __init__(self, alphabet):
		self.alphabet = alphabet
		self.idx2char = list(alphabet) + ['*', '.', '2', ' ', '|']
		self.char2idx = {c: i for i, c in enumerate(self.idx2char)}
		self.unk_idx, self.space_id, self.eps_id = self.char2idx['*'], self.char2idx[' '], self.char2idx['|']

	vocab = property(lambda self: self.idx2char)
	vocab_size = property(lambda self: len(self.idx2char))
	silence_tokens_ids = property(lambda self: {self.eps_id, self.space_id})

	def is_start_word_token(self, idx):
		return idx == self.space_id

	def encode(self, sentences, **kwargs):
		return [[self.char2idx.get(c, self.unk_idx) for c in s] for s in sentences]

	def decode(self, tokens, **kwargs):
		return [''.join(self.idx2char[i] for i in t) for t in tokens]


class GreedyCTCGenerator:
	def __init__(self, blank_amount_to_space = 10):
		self.blank_amount_to_space = blank_amount_to_space

	def device_route(self, tokenizer, log_probs, output_lengths):
		"""Whether generate decodes on the device: CUDA log-probs, lengths as a tensor (or None), an integer blank_amount_to_space >= 0 and a
		tokenizer inside convasr_ctc_greedy_segments' scope -- silence = {eps, space}, and space the one word-start token among the classes."""
		if not (torch.is_tensor(log_probs) and log_probs.is_cuda and log_probs.ndim == 3) or not (output_lengths is None or torch.is_tensor(output_lengths)):
			return False
		eps, space, bats = getattr(tokenizer, 'eps_id', None), getattr(tokenizer, 'space_id', None), self.blank_amount_to_space
		if not all(type(v) is int and v >= 0 for v in (eps, space, bats)) or eps == space or tokenizer.silence_tokens_ids != {eps, space}:
			return False
		return all(bool(tokenizer.is_start_word_token(c)) == (c == space) for c in range(log_probs.shape[1]))

	def generate(self, tokenizer, log_probs, begin, end, output_lengths = None, time_stamps = None, segment_text_key = 'hyp', segment_extra_info = None, uncertainty = False):
		"""uncertainty = True (device route only): every Segment also carries UNCERTAINTY_KEYS -- ops.span_uncertainty over the word's frames and
		over its tokens at their frames, from ONE ops.frame_uncertainty pass whose idx is the decoded path.  uncertainty = (acoustic_log_probs,
		frame_of_position): log_probs are decoded as always, but position p of utterance b stands for frame frame_of_position[b, p] of
		acoustic_log_probs, where the statistics come from (the one-hot targets of --align against the model's own log-probs)."""
		wanted = uncertainty is not False and uncertainty is not None
		if not self.device_route(tokenizer, log_probs, output_lengths):
			if wanted:
				raise ConvasrHipError("GreedyCTCGenerator.generate: uncertainty needs the device decode, and device_route refuses these inputs (it takes CUDA log-probs, lengths as a tensor and a tokenizer of CharTokenizerLegacy's kind)")
			return self.generate_host(tokenizer, log_probs, begin, end, output_lengths, time_stamps, segment_text_key, segment_extra_info)
		B = log_probs.shape[0]
		acoustic = frame_map = stats = None
		if wanted and uncertainty is not True:
			acoustic, frame_map = uncertainty
			stats = ops.frame_uncertainty(acoustic, tokenizer.eps_id)
		elif wanted:
			acoustic, stats = log_probs, ops.frame_uncertainty(log_probs, tokenizer.eps_id, output_lengths)
		path = stats.idx if uncertainty is True else ops.argmax(log_probs)
		tokens, frames, counts, seg_first, seg_begin, seg_end = ops.ctc_greedy_segments(path, output_lengths, tokenizer.eps_id, tokenizer.space_id,
		                                                                                self.blank_amount_to_space, split_words = time_stamps is not None)
		n_seg = counts[1].tolist()
		fields = None
		if wanted and len(seg_first) > 0:
			utt = torch.repeat_interleave(counts[1], output_size = len(seg_first))
			first = torch.cat([seg_first, torch.tensor([len(tokens)], dtype = torch.int64, device = seg_first.device)])
			span = ops.span_uncertainty(acoustic, stats, utt, seg_begin, seg_end, first, tokens, frames, path = path, frame_map = frame_map)
			fields = torch.stack([getattr(span, key) for key in UNCERTAINTY_KEYS]).cpu().tolist()
		tokens, seg_first = tokens.tolist(), seg_first.tolist()
		if time_stamps is not None:  # the stamps of the segments' begin / end frames, gathered where the stamps live
			utt = torch.repeat_interleave(counts[1], output_size = len(seg_first)).to(time_stamps.device)
			at = torch.stack([seg_begin, seg_end]).to(device = utt.device, dtype = torch.int64)
			ts_begin, ts_end = time_stamps[utt, at].cpu().tolist()
			begin = torch.clamp(begin, min = 0.0).cpu().tolist()
		else:
			begin = begin.cpu().tolist()
		end = end.cpu().tolist()
		seg_first.append(len(tokens))
		texts = tokenizer.decode([tokens[seg_first[k]:seg_first[k + 1]] for k in range(len(seg_first) - 1)])
		result, k0 = [], 0
		for i in range(B):
			transcript = Transcript()
			for k in range(k0, k0 + n_seg[i]):
				t_begin, t_end = (begin[i] + ts_begin[k], begin[i] + ts_end[k]) if time_stamps is not None else (begin[i], end[i])
				seg = Segment(begin = t_begin, end = t_end, **{segment_text_key: texts[k]})
				if fields is not None:
					seg.update({key: column[k] for key, column in zip(UNCERTAINTY_KEYS, fields)})
				if segment_extra_info is not None:
					seg.update(segment_extra_info[i])
				transcript.append(seg)
			k0 += n_seg[i]
			result.append([transcript])
		return result

	def generate_host(self, tokenizer, log_probs, begin, end, output_lengths = None, time_stamps = None, segment_text_key = 'hyp', segment_extra_info = None):
		idx_all = (ops.argmax(log_probs) if log_probs.is_cuda else log_probs.argmax(dim = 1)).cpu().tolist()
		ts_all = time_stamps.cpu().tolist() if time_stamps is not None else None
		begin = torch.clamp(begin, min = 0.0).cpu().tolist() if time_stamps is not None else begin.cpu().tolist()
		end = end.cpu().tolist()
		lens = output_lengths.cpu().tolist() if torch.is_tensor(output_lengths) else output_lengths
		silence, eps, space = tokenizer.silence_tokens_ids, tokenizer.eps_id, getattr(tokenizer, 'space_id', None)
		result = []
		for i, path in enumerate(idx_all):
			n = lens[i] if lens is not None else len(path)
			ts = ts_all[i] if ts_all is not None else None
			transcript = Transcript()
			start = next((t for t, c in enumerate(path) if c not in silence), len(path))
			if start >= len(path):
				result.append([transcript])
				continue
			tokens = [eps]
			t_begin = begin[i] + ts[start] if ts is not None else begin[i]
			t_end = end[i]
			blanks, repeat_ok = 0, False

			def flush():
				seg = Segment(begin = t_begin, end = t_end, **{segment_text_key: tokenizer.decode([tokens[1:]])[0]})
				if segment_extra_info is not None:
					seg.update(segment_extra_info[i])
				transcript.append(seg)

			for t in range(start, n):
				c = path[t]
				if c == eps:
					if tokens[-1] == space:
						continue
					repeat_ok = True
					blanks += 1
					if blanks >= self.blank_amount_to_space and not tokenizer.is_start_word_token(tokens[-1]):
						tokens.append(space)
					continue
				if c == tokens[-1] and not repeat_ok:
					continue
				if ts is not None and tokenizer.is_start_word_token(c):
					flush()
					tokens = [eps, c]
					t_begin = begin[i] + ts[t]
				repeat_ok = False
				tokens.append(c)
				t_end = begin[i] + ts[t] if ts is not None else end[i]
				blanks = 0
			if len(tokens) > 1:
				flush()
			result.append([transcript])
		return result


class BeamCTCGenerator:
	"""GreedyCTCGenerator's interface over the CTC prefix beam search (convasr_ctc_beam_search; the reference's transcribe.py
	--decoder BeamSearchDecoder; with lm_path an ARPA n-gram model fused as --lm / --beam-alpha / --beam-beta do, convasr_ctc_beam_search_lm,
	the labels being the tokenizer's characters).  Per utterance it returns topk alternatives, best first; each is a Transcript
	of word segments built from that beam's tokens: leading silence tokens are skipped, a new segment starts at every word-start token
	when time stamps are given, and a token's time is begin + time_stamps[its frame offset].  GPU only: log_probs must be a CUDA tensor
	(GreedyCTCGenerator also decodes CPU tensors); for the one-hot targets of --align, transcribe_batch uses a GreedyCTCGenerator.
	beam_width up to 8192 (the reference's default --beam-width 5000 runs the wide kernel: decoders.BeamSearchDecoder).
	hotwords (a list of phrases) with hotword_weight (required with them, no default) bias the search towards the phrases
	(decoders.BeamSearchDecoder, convasr_ctc_beam_search_hot); the tokenizer's vocabulary then needs exactly one space."""

	def __init__(self, beam_width = 64, topk = 1, cutoff_top_n = 40, cutoff_prob = 1.0, lm_path = None, beam_alpha = 0, beam_beta = 0, hotwords = None, hotword_weight = None):
		from . import decoders, lm
		self.topk = int(topk)
		kw = dict(beam_width = beam_width, cutoff_top_n = cutoff_top_n, cutoff_prob = cutoff_prob, topk = topk)
		if (hotwords is None) != (hotword_weight is None):
			raise ValueError('BeamCTCGenerator: hotwords and hotword_weight go together (there is no default weight)')
		if lm_path is None and hotwords is None:
			self.decoder = lambda tokenizer: decoders.BeamSearchDecoder(types.SimpleNamespace(blank_idx = tokenizer.eps_id), **kw)
			self.decoder(types.SimpleNamespace(eps_id = 0))
			return
		model = lm_path if lm_path is None or isinstance(lm_path, lm.NgramLM) else lm.read_arpa(lm_path)  # (a non-ARPA path raises here, at setup)
		decs = {}

		def decoder(tokenizer):  # one decoder (one set of LM tables, one hot-phrase trie) per tokenizer alphabet
			labels = ''.join(tokenizer.vocab)
			if (labels, tokenizer.eps_id) not in decs:
				decs[labels, tokenizer.eps_id] = decoders.BeamSearchDecoder(types.SimpleNamespace(eps_id = tokenizer.eps_id, idx2char = tokenizer.vocab), lm_path = model,
				                                                            beam_alpha = beam_alpha, beam_beta = beam_beta, hotwords = hotwords, hotword_weight = hotword_weight, **kw)
			return decs[labels, tokenizer.eps_id]
		self.decoder = decoder

	def generate(self, tokenizer, log_probs, begin, end, output_lengths = None, time_stamps = None, segment_text_key = 'hyp', segment_extra_info = None, uncertainty = False):
		"""uncertainty = True: every Segment also carries UNCERTAINTY_KEYS (ops.span_uncertainty).  A word's span runs from its first token's
		frame offset to its last one's and its events are its tokens at their offsets; a beam's token need not be its frame's argmax, so a
		word's margin can be negative.  The spans of all alternatives are built in the host loop and uploaded once."""
		tokens, offsets, lengths, _ = self.decoder(tokenizer).decode_with_scores(log_probs, output_lengths)
		tokens, offsets, lengths = tokens.cpu().tolist(), offsets.cpu().tolist(), lengths.cpu().tolist()
		spans = dict(segments = [], utt = [], begin = [], end = [], first = [0], tokens = [], frames = []) if uncertainty else None
		ts_all = time_stamps.cpu().tolist() if time_stamps is not None else None
		begin = torch.clamp(begin, min = 0.0).cpu().tolist() if time_stamps is not None else begin.cpu().tolist()
		end = end.cpu().tolist()
		silence = tokenizer.silence_tokens_ids
		result = []
		for i in range(len(tokens)):
			ts = ts_all[i] if ts_all is not None else None
			alternatives = []
			for k in range(self.topk):
				toks, offs = tokens[i][k][:lengths[i][k]], offsets[i][k][:lengths[i][k]]
				transcript = Transcript()
				start = next((j for j, c in enumerate(toks) if c not in silence), len(toks))
				at = lambda j: begin[i] + ts[offs[j]] if ts is not None else None
				seg_tokens, t_begin, t_end = [], at(start) if ts is not None and start < len(toks) else begin[i], end[i]
				j_first = start

				def flush(j_end):
					seg = Segment(begin = t_begin, end = t_end, **{segment_text_key: tokenizer.decode([seg_tokens])[0]})
					if spans is not None:  # the word = tokens [j_first, j_end) of this beam
						spans['segments'].append(seg)
						spans['utt'].append(i)
						spans['begin'].append(offs[j_first])
						spans['end'].append(offs[j_end - 1])
						spans['tokens'] += toks[j_first:j_end]
						spans['frames'] += offs[j_first:j_end]
						spans['first'].append(len(spans['tokens']))
					if segment_extra_info is not None:
						seg.update(segment_extra_info[i])
					transcript.append(seg)

				for j in range(start, len(toks)):
					c = toks[j]
					if ts is not None and tokenizer.is_start_word_token(c) and seg_tokens:
						flush(j)
						seg_tokens, t_begin, j_first = [], at(j), j
					seg_tokens.append(c)
					t_end = at(j) if ts is not None else end[i]
				if seg_tokens:
					flush(len(toks))
				alternatives.append(transcript)
			result.append(alternatives)
		if spans is not None and spans['segments']:
			stats = ops.frame_uncertainty(log_probs, tokenizer.eps_id, output_lengths)
			span = ops.span_uncertainty(log_probs, stats, spans['utt'], spans['begin'], spans['end'], spans['first'], spans['tokens'], spans['frames'])
			fields = torch.stack([getattr(span, key) for key in UNCERTAINTY_KEYS]).cpu().tolist()
			for k, seg in enumerate(spans['segments']):
				seg.update({key: column[k] for key, column in zip(UNCERTAINTY_KEYS, fields)})
		return result
