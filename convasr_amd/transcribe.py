"""MI355X-native mirror of the model-facing surface of the reference's transcribe.py.

* setup(args) -> (text_pipeline, frontend, model, generator)                          transcribe.py:23-60
  checkpoint -> frontend + model (the reference's class names / state-dict keys) -> eval() -> fuse_conv_bn_eval() ->
  compute dtype from args.fp16 (None / 'O0': exact fp32; 'O1'..'O3': fp16 storage + MFMA as under apex.amp, or bf16 when models.AMP_DTYPE says so) -> greedy generator,
  or with args.decoder = 'BeamSearchDecoder' the CTC prefix beam search (args.beam_width, args.decoder_topk; args.lm an ARPA n-gram model
  weighed by args.beam_alpha / args.beam_beta; args.hotwords, a list of phrases or the path of a text file with one phrase per line, and
  args.hotword_weight bias the search towards those phrases: this package's own, the reference has no hot words).
* transcribe_batch(...)                                                                transcribe.py:140-200
  the per-batch body of transcribe.main: forward (every op a HIP kernel; the argmax of the greedy decode too), per-frame time
  stamps, GreedyCTCGenerator with time stamps (one segment per word), optional forced alignment of the reference text
  (ctc.alignment on the GPU) -> ref segments.
* transcribe_file(...) / transcribe_long(...)
  transcribe_batch on a wav / raw file: every channel as one row, or -- for a long recording -- the speech cut at silences (vad.segments) or
  at given segments and gathered into padded batches on the GPU, the words back on the recording's clock.
* search_batch(...) / search_long(...)
  this package's own (the reference has no keyword search): where phrases are SAID in a batch or in a long recording -- the model call of
  transcribe_batch, then ctc.search_bct on its log-probs (ops.ctc_keyword_search: the CTC lattice of every phrase started at every frame,
  scored against the greedy path), hits as segments on the same clock as the words.

Out of scope: file discovery, audio decoding, the dataset, text pre/post-processing pipelines (regexes, number
normalisation) and the json / html / csv / txt writers around this body (CER and the error analysis live in metrics).  A TextPipeline here is the tokenizer
plus identity pre/post-processing; pass the reference's own pipeline object as args.text_pipeline to get its text handling."""
import os
import types

import torch

from . import ctc, models
from .transcript_generators import BeamCTCGenerator, CharTokenizerLegacy, GreedyCTCGenerator, Segment

RU_ALPHABET = 'абвгдеёжзийклмнопрстуфхцчшщъыьэюя'  # configs/ru_text_config.json:10


class TextPipeline:
	"""What transcribe.py uses of text_processing.ProcessingPipeline: .tokenizer, .preprocess, .postprocess."""

	def __init__(self, tokenizer, preprocess = None, postprocess = None):
		self.tokenizer = tokenizer
		self.preprocess = preprocess or (lambda s: s)
		self.postprocess = postprocess or (lambda s: s)


def map_text(postprocess, hyp = (), ref = ()):
	"""transcripts.map_text (transcripts.py:34-35)."""
	return [dict(t, hyp = postprocess(t.get('hyp', ''))) for t in hyp] + [dict(t, ref = postprocess(t.get('ref', ''))) for t in ref]


def join(ref = (), hyp = ()):
	"""transcripts.join (transcripts.py:82-83)."""
	return ' '.join(filter(bool, [t.get('ref', '').strip() for t in ref] + [t.get('hyp', '').strip() for t in hyp]))


def _hotwords_of(args):
	"""args.hotwords: None, a list of phrases, or the path of a text file with one phrase per line."""
	hot = getattr(args, 'hotwords', None)
	if isinstance(hot, (str, os.PathLike)):
		from . import hotwords
		hot = hotwords.read_phrases(hot)
	return hot


def setup(args):
	"""transcribe.setup(args).  args: namespace with checkpoint (a path, or the dict torch.load would return: 'args' and
	'model_state_dict'), device, fp16 (apex opt level or None), frontend_in_model, model (optional override), dither / dither0 /
	normalize_signal (optional), text_pipeline (optional; default: the legacy 38-symbol character tokenizer).
	An API mirror of ONE ~30-line reference function (transcribe.py:23-60): the order of its statements -- checkpoint args into `args`, frontend,
	text pipeline, model by class name, load_state_dict, eval / fuse / autocast, generator -- is the reference's, because a caller of the
	reference observes each of them (mutated args, loaded keys); the arithmetic behind every call is this package's."""
	torch.set_grad_enabled(False)
	checkpoint = args.checkpoint if isinstance(args.checkpoint, dict) else torch.load(args.checkpoint, map_location = 'cpu')
	args.sample_rate, args.window_size, args.window_stride, args.window, args.num_input_features = map(checkpoint['args'].get, ['sample_rate', 'window_size', 'window_stride', 'window', 'num_input_features'])
	frontend = models.LogFilterBankFrontend(
		args.num_input_features, args.sample_rate, args.window_size, args.window_stride, args.window,
		dither = getattr(args, 'dither', 0.0), dither0 = getattr(args, 'dither0', 0.0), normalize_signal = getattr(args, 'normalize_signal', True),
		debug_short_long_records_normalize_signal_multiplier = getattr(args, 'debug_short_long_records_normalize_signal_multiplier', 1.0))
	text_pipeline = getattr(args, 'text_pipeline', None) or TextPipeline(CharTokenizerLegacy(checkpoint['args'].get('alphabet', RU_ALPHABET)))
	model = getattr(models, getattr(args, 'model', None) or checkpoint['args']['model'])(
		args.num_input_features, [text_pipeline.tokenizer.vocab_size],
		frontend = frontend if getattr(args, 'frontend_in_model', True) else None,
		check_time_dim_padded = False,
		dict = lambda logits, log_probs, olen, **kwargs: (log_probs[0], logits[0], olen[0]),
		**checkpoint['args'].get('model_kwargs', {}))
	model.load_state_dict(checkpoint['model_state_dict'], strict = False)
	model = model.to(args.device)
	model.eval()
	model.fuse_conv_bn_eval()
	if str(args.device) != 'cpu':
		level = getattr(args, 'fp16', None)
		if level in models.JasperNet.SPLIT_DTYPES:  # (this package's own: args.fp16 = 'bf16x3' / 'f16x3' -- fp32-class logits from split-operand convs on the 16-bit matrix pipe)
			models.master_module(model).set_compute_dtype(level, inference = True)
		else:
			model, *_ = models.data_parallel_and_autocast(model, opt_level = level)
	if getattr(args, 'decoder', None) == 'BeamSearchDecoder':  # transcribe.py:323-328: --decoder, --beam-width, --decoder-topk, --lm (an ARPA file), --beam-alpha, --beam-beta
		generator = BeamCTCGenerator(beam_width = args.beam_width, topk = getattr(args, 'decoder_topk', 1), lm_path = getattr(args, 'lm', None),
		                             beam_alpha = getattr(args, 'beam_alpha', 0), beam_beta = getattr(args, 'beam_beta', 0),
		                             hotwords = _hotwords_of(args), hotword_weight = getattr(args, 'hotword_weight', None))
	else:
		generator = GreedyCTCGenerator()
	return text_pipeline, frontend, model, generator


def _forward(args, model, x, xlen):
	"""The model call of transcribe_batch and search_batch and the per-frame time stamps (transcribe.py:150-160): x (B, 1, T) or (B, T) waveform,
	xlen (B,) fractions -> log_probs, logits, olen, ts (B, frames) seconds from the batch's first sample."""
	device = torch.device(args.device)
	x = x.squeeze(1) if x.ndim == 3 else x
	log_probs, logits, olen = model(x.to(device), xlen.to(device))
	duration = x.shape[-1] / args.sample_rate
	ts = duration * torch.linspace(0, 1, steps = log_probs.shape[-1], device = log_probs.device).unsqueeze(0).expand(x.shape[0], -1)
	return log_probs, logits, olen, ts


def transcribe_batch(args, text_pipeline, model, generator, x, xlen, begin, end, y = None, ylen = None, segment_extra_info = None):
	"""One iteration of transcribe.main's loop (transcribe.py:140-200) on a collated batch: x (B, 1, T) or (B, T) waveform,
	xlen (B,) fractions, begin / end (B,) seconds, optional targets y (B, L, S) / ylen (B, L) for --align.
	Returns a namespace: log_probs, logits, olen, ts (per-frame time stamps), hyp_segments (per utterance: list of word segments with
	begin / end / hyp), hyp (joined strings) and, when args.align and targets are given, alignment (B, S), ref_segments.
	args.align_star = ctc.StarCTC(...) (absent = off; with args.align and targets): the alignment is StarCTC.align's -- the transcript may miss
	words --, alignment and ref_segments are formed from it as before, and star_segments (per utterance: Segment(begin, end, gap, frames) on
	the batch's clock for the stars of at least args.align_star_min_frames frames, default 1) and ref_pieces (ctc.star_pieces' pieces:
	Segment(begin, end, first_label, label_count), seconds) are added; both are None otherwise.
	args.uncertainty (absent = off): every hyp and ref word segment also carries confidence, confidence_min, margin, entropy, uncertainty
	(GreedyCTCGenerator / BeamCTCGenerator.generate's uncertainty; transcribe_file and transcribe_long pass args on, and transcribe_long's words keep the fields).
	When args.align_words is set and targets are given, also ref (the decoded, postprocessed targets) and words: per utterance
	metrics.align_words(*metrics.align_strings(hyp = hyp, ref = ref)) (transcribe.py:235), the strings of the whole batch aligned in two
	GPU launches; words is None otherwise."""
	device = torch.device(args.device)
	log_probs, logits, olen, ts = _forward(args, model, x, xlen)
	tokenizer = text_pipeline.tokenizer
	with_uncertainty = bool(getattr(args, 'uncertainty', False))  # every word segment also carries transcript_generators.UNCERTAINTY_KEYS
	hyp_segments = [alternatives[0] for alternatives in generator.generate(tokenizer = tokenizer, log_probs = log_probs, begin = begin, end = end, output_lengths = olen, time_stamps = ts, segment_text_key = 'hyp', segment_extra_info = segment_extra_info, **(dict(uncertainty = True) if with_uncertainty else {}))]
	hyp_segments = [map_text(text_pipeline.postprocess, hyp = hyp) for hyp in hyp_segments]
	out = types.SimpleNamespace(log_probs = log_probs, logits = logits, olen = olen, ts = ts, hyp_segments = hyp_segments, hyp = [join(hyp = h) for h in hyp_segments], alignment = None, ref_segments = None, ref = None, words = None, star_segments = None, ref_pieces = None)
	if getattr(args, 'align', False) and y is not None and y.numel() > 0:
		y, ylen = y.to(device), ylen.to(device)
		star = getattr(args, 'align_star', None)
		if star is not None:  # a transcript with holes: the stars take the audio it does not cover, the labels keep their own frames
			result = star.align(log_probs, y[:, 0, :], olen, ylen[:, 0], blank = tokenizer.eps_id)
			out.alignment = result.alignment
			out.star_segments, out.ref_pieces = [], []
			for row, found in zip(ts.tolist(), ctc.star_pieces(result, y[:, 0, :], ylen[:, 0], getattr(args, 'align_star_min_frames', 1))):
				out.star_segments.append([Segment(begin = row[lo], end = row[hi], gap = g, frames = hi - lo + 1) for g, lo, hi in found.stars])
				out.ref_pieces.append([Segment(begin = row[lo], end = row[hi], first_label = first, label_count = count) for first, count, lo, hi in found.pieces])
		else:
			align = ctc.alignment_long_bct if y.shape[-1] > 8191 else ctc.alignment_bct  # (a whole recording against its transcript: past ctc.alignment's 8,191 labels)
			out.alignment = align(log_probs, y[:, 0, :], olen, ylen[:, 0], blank = tokenizer.eps_id)
		aligned_ts = ts.gather(1, out.alignment)
		one_hot = torch.nn.functional.one_hot(y[:, 0, :], num_classes = log_probs.shape[1]).permute(0, 2, 1).to(torch.float32)
		ref_generator = generator if isinstance(generator, GreedyCTCGenerator) else GreedyCTCGenerator()  # one-hot targets: the argmax collapse gives back y; a beam search over 0 / 1 "log-probs" would not
		ref_segments = [alternatives[0] for alternatives in ref_generator.generate(tokenizer = tokenizer, log_probs = one_hot, begin = begin, end = end, output_lengths = ylen[:, 0], time_stamps = aligned_ts, segment_text_key = 'ref', segment_extra_info = segment_extra_info,
		                                                                           # a reference word's fields: what the MODEL gives its tokens at their aligned frames (a transcript that does not match the audio shows as low confidence)
		                                                                           **(dict(uncertainty = (log_probs, out.alignment)) if with_uncertainty else {}))]
		out.ref_segments = [map_text(text_pipeline.postprocess, ref = ref) for ref in ref_segments]
	if getattr(args, 'align_words', False) and y is not None and y.numel() > 0:
		from . import metrics
		out.ref = [text_pipeline.postprocess(tokenizer.decode([row[:n]])[0].strip()) for row, n in zip(y[:, 0].tolist(), ylen[:, 0].tolist())]
		aligned = metrics.align_strings_batch(out.hyp, out.ref)
		out.words = [metrics.align_words(_hyp_, _ref_) for _hyp_, _ref_ in aligned]
	return out


def transcribe_file(args, text_pipeline, model, generator, audio_path, **read_audio_kwargs):
	"""transcribe_batch on a wav / raw file instead of a tensor: audio.read_audio at args.sample_rate and args.mono (default True) -- decode, mono
	mix and the change of sample rate on the GPU -- then every channel of the result as one utterance of the batch (transcribe.py:140-200 over
	the reference's per-channel batches)."""
	from . import audio
	signal, sample_rate = audio.read_audio(audio_path, args.sample_rate, mono = getattr(args, 'mono', True), device = args.device, **read_audio_kwargs)
	channels, duration = signal.shape[0], signal.shape[1] / sample_rate
	return transcribe_batch(args, text_pipeline, model, generator, signal, torch.ones(channels), torch.zeros(channels), torch.full((channels, ), duration))


def _long_batches(args, audio_or_signal, segments, read_audio_kwargs):
	"""What transcribe_long and search_long share (their docstrings have the rules): the recording read, cut into segments (by channel, then
	time) and gathered into padded batches, longest segments first.  Returns (channels, segments, batches); batches yields, per chunk of
	args.batch_size segments, (their indices into segments, x, xlen, begin, end, segment_extra_info) as transcribe_batch takes them."""
	from . import audio, ops, vad
	if torch.is_tensor(audio_or_signal):
		signal, sample_rate = audio_or_signal, args.sample_rate
	else:
		signal, sample_rate = audio.read_audio(audio_or_signal, args.sample_rate, mono = getattr(args, 'mono', True), device = args.device, **read_audio_kwargs)
	channels, N = signal.shape
	if segments is None:
		segments = vad.segments(signal, sample_rate, window_size = getattr(args, 'vad_window_size', 0.02), aggressiveness = getattr(args, 'vad_aggressiveness', 2),
		                        max_duration = getattr(args, 'vad_max_duration', 15.0))
	else:
		given, segments = segments, []
		for s in given:
			first, count = vad.segment_samples(s['begin'], s['end'], sample_rate, N)
			segments.append(dict(s, first = first, count = count))
		segments.sort(key = lambda s: (s['channel'], s['first']))
	order = sorted(range(len(segments)), key = lambda i: -segments[i]['count'])
	batch_size, multiple = getattr(args, 'batch_size', 64), getattr(args, 'batch_time_padding_multiple', 128)

	def batches():
		for at in range(0, len(order), batch_size):
			idx = order[at:at + batch_size]
			chunk = [segments[i] for i in idx]
			x, xlen = ops.gather_segments(signal, [s['channel'] for s in chunk], [s['first'] for s in chunk], [s['count'] for s in chunk], multiple = multiple)
			yield (idx, x, xlen, torch.tensor([s['begin'] for s in chunk], dtype = torch.float64), torch.tensor([s['end'] for s in chunk], dtype = torch.float64),
			       [dict(channel = s['channel']) for s in chunk])
	return channels, segments, batches()


def transcribe_long(args, text_pipeline, model, generator, audio_or_signal, segments = None, **read_audio_kwargs):
	"""A long recording as batches of utterance-sized segments instead of transcribe_file's one row per channel: the audio is read with
	audio.read_audio at args.sample_rate and args.mono (default True) unless a (C, N) device tensor is given; it is cut into segments; the
	segments, longest first (a stable sort by their sample counts), go in chunks of args.batch_size (default 64) through ops.gather_segments
	-- one zero-padded batch per launch, padded to args.batch_time_padding_multiple (default 128) -- and transcribe_batch, with begin / end the
	segments' seconds (float64 tensors: the Python floats as they are), so every word carries a time on the recording's clock, and its channel.
	segments: None = vad.segments with args.vad_aggressiveness (default 2), args.vad_window_size (0.02) and args.vad_max_duration (15.0).  A list
	of dicts with begin, end, channel -- a reference transcript (the reference's batched_transcript mode, datasets.py:261-262), or
	diarization.diarize's output with channel = speaker - 1 -- is sliced by vad.segment_samples instead.
	Returns a namespace: segments (dicts with begin, end, channel, first, count; by channel, then time), hyp_segments and hyp per segment in that
	order, transcript (all word segments sorted by begin, end, channel) and text (per channel, the joined hypothesis in time order).  A
	recording without speech returns empty lists and does not call the model."""
	channels, segments, batches = _long_batches(args, audio_or_signal, segments, read_audio_kwargs)
	hyp_segments, hyp = [None] * len(segments), [None] * len(segments)
	for idx, x, xlen, begin, end, extra in batches:
		out = transcribe_batch(args, text_pipeline, model, generator, x, xlen, begin, end, segment_extra_info = extra)
		for i, words, text in zip(idx, out.hyp_segments, out.hyp):
			hyp_segments[i], hyp[i] = words, text
	transcript = sorted((w for words in hyp_segments for w in words), key = lambda w: (w['begin'], w['end'], w['channel']))
	by_time = sorted(range(len(segments)), key = lambda i: (segments[i]['begin'], segments[i]['end']))
	text = [join(hyp = [dict(hyp = hyp[i]) for i in by_time if segments[i]['channel'] == c]) for c in range(channels)]
	return types.SimpleNamespace(segments = list(segments), hyp_segments = hyp_segments, hyp = hyp, transcript = transcript, text = text)


def encode_phrases(text_pipeline, phrases):
	"""Phrases as search_batch searches them: text_pipeline.preprocess, then tokenizer.encode.  Returns (texts, label lists).  ValueError for an
	empty list, a phrase that is empty or does not come back from tokenizer.decode as it went in (CharTokenizerLegacy maps a character outside
	its alphabet to '*'), one that holds the blank, and one of more labels than the kernel takes (64)."""
	from . import ops
	tokenizer = text_pipeline.tokenizer
	texts = [text_pipeline.preprocess(p) for p in phrases]
	if not texts:
		raise ValueError('search: no phrases')
	labels = [list(row) for row in tokenizer.encode(texts)]
	limit = ops.ctc_keyword_search_limits()[0]
	for phrase, text, row in zip(phrases, texts, labels):
		if not row or tokenizer.eps_id in row or tokenizer.decode([row])[0] != text:
			raise ValueError(f'search: the phrase {phrase!r} cannot be encoded with this tokenizer')
		if len(row) > limit:
			raise ValueError(f'search: the phrase {phrase!r} has {len(row)} labels, at most {limit} can be searched')
	return texts, labels


def search_batch(args, text_pipeline, model, x, xlen, begin, end, phrases, threshold_per_label = -1.0, min_gap_seconds = 0.2, segment_extra_info = None):
	"""Where each of `phrases` is said in a collated batch (x, xlen, begin, end as transcribe_batch takes them): one model call, one
	ctc.search_bct over its log-probs with the blank tokenizer.eps_id, thresholds[k] = threshold_per_label * (labels of phrase k) and min_gap =
	min_gap_seconds in frames (rounded).  A phrase's spaces are ordinary labels: the model has to emit them.
	Returns a namespace: log_probs, logits, olen, ts, found (ops.ctc_keyword_search's namespace, device tensors), phrases (the preprocessed
	texts) and hits: per utterance a list of Segment(begin, end, phrase, score, score_per_label, **segment_extra_info[b]) sorted by begin, end
	and the phrase's position in the list.  Times follow the greedy generator's convention, max(begin[b], 0) + ts[b, frame] at the hit's first
	and last frame.  score is the acoustic log-likelihood ratio of the best alignment against the greedy path (0 = the greedy path says the
	phrase there), not a calibrated probability."""
	from .transcript_generators import Segment
	texts, labels = encode_phrases(text_pipeline, phrases)
	log_probs, logits, olen, ts = _forward(args, model, x, xlen)
	B, _, T = log_probs.shape
	K, lens = len(labels), [len(row) for row in labels]
	tokens = torch.tensor([row + [0] * (max(lens) - len(row)) for row in labels], dtype = torch.int32)
	duration = x.shape[-1] / args.sample_rate
	min_gap = int(round(min_gap_seconds * (T - 1) / duration)) if T > 1 and duration > 0 else 0
	found = ctc.search_bct(log_probs, tokens, torch.tensor(lens, dtype = torch.int32), text_pipeline.tokenizer.eps_id,
	                       torch.tensor([threshold_per_label * n for n in lens], dtype = torch.float32), lengths = olen, min_gap = min_gap)
	H = found.score.shape[2]
	stored = (torch.arange(H, device = found.count.device) < found.count.unsqueeze(-1)).nonzero()  # (hits, 3): utterance, phrase, slot -- in that order
	b_idx, k_idx, j_idx = stored.unbind(1)
	first, last = found.begin[b_idx, k_idx, j_idx].long(), found.end[b_idx, k_idx, j_idx].long()
	t_begin, t_end = ts[b_idx, first].cpu().tolist(), ts[b_idx, last].cpu().tolist()
	scores, begin = found.score[b_idx, k_idx, j_idx].cpu().tolist(), torch.clamp(begin, min = 0.0).cpu().tolist()
	hits = [[] for _ in range(B)]
	for b, k, tb, te, sc in zip(b_idx.tolist(), k_idx.tolist(), t_begin, t_end, scores):
		hit = Segment(begin = begin[b] + tb, end = begin[b] + te, phrase = texts[k], score = sc, score_per_label = sc / lens[k])
		if segment_extra_info is not None:
			hit.update(segment_extra_info[b])
		hits[b].append((hit['begin'], hit['end'], k, hit))
	hits = [[h[3] for h in sorted(row, key = lambda h: h[:3])] for row in hits]
	return types.SimpleNamespace(log_probs = log_probs, logits = logits, olen = olen, ts = ts, found = found, phrases = texts, hits = hits)


def search_long(args, text_pipeline, model, audio_or_signal, phrases, segments = None, threshold_per_label = -1.0, min_gap_seconds = 0.2, **read_audio_kwargs):
	"""search_batch over a long recording: the segmenting and batching are transcribe_long's (its docstring has the rules; segments = None cuts
	at silences, a list of dicts with begin, end, channel is sliced as given), every batch goes through search_batch with the segments' seconds
	as begin / end and their channel as extra field.  A phrase is found only inside a segment: one that straddles a cut is not.
	Returns a namespace: segments (as transcribe_long's), hits_per_segment in that order and hits: every hit, on the recording's clock and with
	its channel, sorted by (begin, end, channel).  A phrase that cannot be encoded or has more than 64 labels raises ValueError before the audio
	is read; a recording without speech returns empty lists and does not call the model."""
	encode_phrases(text_pipeline, phrases)
	channels, segments, batches = _long_batches(args, audio_or_signal, segments, read_audio_kwargs)
	per_segment = [None] * len(segments)
	for idx, x, xlen, begin, end, extra in batches:
		out = search_batch(args, text_pipeline, model, x, xlen, begin, end, phrases, threshold_per_label = threshold_per_label, min_gap_seconds = min_gap_seconds, segment_extra_info = extra)
		for i, found in zip(idx, out.hits):
			per_segment[i] = found
	hits = sorted((h for found in per_segment for h in found), key = lambda h: (h['begin'], h['end'], h['channel']))
	return types.SimpleNamespace(segments = list(segments), hits_per_segment = per_segment, hits = hits)
