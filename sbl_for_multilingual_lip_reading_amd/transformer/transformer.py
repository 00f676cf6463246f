"""Transformer: the reference's top-level model class (transformer/transformer.py surface), frontend + encoder +
bidirectional decoder."""
import torch
import torch.nn as nn

from ._env import ops
from .video_frontend import visual_frontend


class Transformer(nn.Module):
    """Lip crops -> visual frontend -> encoder -> SBL decoder.  Construction re-draws every parameter of rank >= 2
    Xavier-uniform, in registration order (as the reference does; biases and norm affines keep their init)."""

    def __init__(self, encoder, decoder, pt):
        super(Transformer, self).__init__()
        self.visual_frontend = visual_frontend(pt)
        self.encoder = encoder
        self.decoder = decoder
        for w in [p for p in self.parameters() if p.dim() >= 2]:
            nn.init.xavier_uniform_(w)

    def _encode(self, frames, input_lengths=None):
        """frames (N, T, H, W) grayscale, or an ops.RawClips of that logical shape (the loader's uint8 frames: no float clip is
        built) -> (encoder output (N, T, 512), lengths).  input_lengths = None: every clip uses all its frames (the reference
        passes full lengths too); else the device int32 (N,) frame counts of `_lengths` (inference): the frames behind a
        clip's count must be all-zero frames (RawClips.src_frame = -1, what the loader pads with), which is what the stem's
        temporal zero padding gives the clip cut to its count, and the encoder keeps them out of its attention."""
        if not isinstance(frames, ops.RawClips):
            frames = frames.unsqueeze(1)                        # (N, 1, T, H, W): one input channel
        feats = self.visual_frontend(frames)
        lengths = [feats.size(1)] * feats.size(0) if input_lengths is None else input_lengths
        enc, *_ = self.encoder(feats, lengths)
        return enc, lengths

    @staticmethod
    def _lengths(input, input_lengths):
        """The `input_lengths` argument of the inference methods -> None or a device int32 (N,) tensor.  A host sequence or
        CPU tensor is checked here, before anything runs (N entries, 1 <= l <= T), and copied to the device once; a CUDA
        int32 tensor is used as it is, never read on the host, and may be overwritten in place between replays of a captured
        graph (the kernels clamp a count to 0..T)."""
        if input_lengths is None:
            return None
        N, T = int(input.shape[0]), int(input.shape[1])
        if isinstance(input_lengths, torch.Tensor) and input_lengths.is_cuda:
            if input_lengths.dtype != torch.int32 or input_lengths.shape != (N,) or not input_lengths.is_contiguous():
                raise ValueError("input_lengths on the device must be a contiguous int32 (%d,) tensor, got %s %s"
                                 % (N, input_lengths.dtype, tuple(input_lengths.shape)))
            return input_lengths
        lens = [int(l) for l in (input_lengths.tolist() if isinstance(input_lengths, torch.Tensor) else input_lengths)]
        if len(lens) != N:
            raise ValueError("input_lengths has %d entries for %d clips" % (len(lens), N))
        if any(not 1 <= l <= T for l in lens):
            raise ValueError("input_lengths %s outside 1..T = %d" % (lens, T))
        dev = input.frames_u8.device if isinstance(input, ops.RawClips) else input.device
        return torch.tensor(lens, dtype=torch.int32).to(dev)

    def forward(self, padded_input, padded_target_l2r, padded_target_r2l):
        """padded_input (N, T, H, W) or ops.RawClips; targets (N, To), IGNORE_ID padded.
        Returns (pred_l2r (N, 16, 58), gold_l2r (N, 16), pred_r2l, gold_r2l)."""
        enc, lengths = self._encode(padded_input)
        return self.decoder(padded_target_l2r, padded_target_r2l, enc, lengths)

    def recognize(self, input, input_lengths=None):
        """Greedy bidirectional decode of (N, T, H, W) crops (or ops.RawClips): (ys_l2r, ys_r2l), int64 (N, 17).
        input_lengths (here and in every inference method below; gradients disabled): None, or the clips' frame counts (N ints,
        or a device int32 (N,) tensor: `_lengths`).  Clip n then decodes as it would alone, cut to its first input_lengths[n]
        frames; its frames behind the count must be all-zero frames."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        return self.decoder.recognize_beam(enc, lens)

    def recognize_nbest(self, input, beam_size, nbest=1, input_lengths=None):
        """Beam-search decode of (N, T, H, W) crops (or ops.RawClips) over pairs of an l2r and an r2l hypothesis:
        Decoder.beam_search on the encoder output -> PairBeamResult, the nbest best pairs of every clip, best first."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        return self.decoder.beam_search(enc, beam_size, nbest, lens)

    def validate(self, padded_input, padded_target_l2r, padded_target_r2l, meter, valid_rows=None, beam_size=None,
                 input_lengths=None):
        """One validation batch (the body of valid_lrw's loop, train.py:236-276): greedy decode, then score both directions
        against the (N, To) IGNORE_ID-padded targets into `meter` (metrics.ErrorRateMeter) on the device.  No host sync:
        in eval() under torch.no_grad() the whole call is capturable as one hipGraph, like recognize; `valid_rows` (device
        int32[1]) then masks the tail of a short last batch.  Returns the token tensors of recognize.
        With beam_size the decode is the beam search (recognize_nbest) and the scored tokens are its best pair's."""
        if beam_size is not None:
            res = self.recognize_nbest(padded_input, beam_size, 1, input_lengths)
            ys_l2r, ys_r2l = res.ys_l2r[:, 0].contiguous(), res.ys_r2l[:, 0].contiguous()
        else:
            ys_l2r, ys_r2l = self.recognize(padded_input, input_lengths)
        meter.update(ys_l2r, ys_r2l, padded_target_l2r, padded_target_r2l, valid_rows=valid_rows)
        return ys_l2r, ys_r2l

    def recognize_words(self, input, lexicon, beam_size=None, nbest=1, shortlist=8, input_lengths=None):
        """Closed-vocabulary decode of (N, T, H, W) crops (or ops.RawClips): Decoder.recognize_words on the encoder output ->
        WordResult, the lexicon word of every clip with its shortlist and the shortlist's pair scores."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        return self.decoder.recognize_words(enc, lexicon, beam_size=beam_size, nbest=nbest, shortlist=shortlist,
                                            encoder_input_lengths=lens)

    def validate_words(self, padded_input, gold_word, lexicon, meter, valid_rows=None, beam_size=None, nbest=1, shortlist=8,
                       input_lengths=None):
        """One validation batch of a closed-vocabulary benchmark: recognize_words, then `meter` (metrics.WordAccuracyMeter)
        counts the clips whose word is gold_word (N,) int64 - word indices into `lexicon`, as Lexicon.from_targets returns
        them - and those whose shortlist holds it.  No host sync: in eval() under torch.no_grad() the call is capturable as
        one hipGraph; `valid_rows` (device int32[1]) masks the tail of a short last batch.  Returns the WordResult."""
        res = self.recognize_words(padded_input, lexicon, beam_size=beam_size, nbest=nbest, shortlist=shortlist,
                                   input_lengths=input_lengths)
        meter.update(res, gold_word, valid_rows=valid_rows)
        return res

    def recognize_words_lex(self, input, lexicon, beam_size, nbest=1, input_lengths=None):
        """Closed-vocabulary decode of (N, T, H, W) crops (or ops.RawClips) in one pass: Decoder.beam_search_lex on the encoder
        output -> PairWordBeamResult, the nbest best lexicon words of every clip by the model's own pair score."""
        lens = self._lengths(input, input_lengths)
        enc, _ = self._encode(input, lens)
        return self.decoder.beam_search_lex(enc, lexicon, beam_size, nbest, lens)

    def validate_words_lex(self, padded_input, gold_word, lexicon, meter, valid_rows=None, beam_size=8, nbest=1,
                           input_lengths=None):
        """validate_words through the lexicon-constrained pair beam search (recognize_words_lex): `meter`
        (metrics.WordAccuracyMeter, unchanged) counts the clips whose word is gold_word, and as n_in_shortlist those whose
        n-best words hold it.  No host sync: capturable as one hipGraph in eval() under torch.no_grad(); `valid_rows` (device
        int32[1]) masks the tail of a short last batch.  Returns the PairWordBeamResult."""
        res = self.recognize_words_lex(padded_input, lexicon, beam_size, nbest, input_lengths)
        meter.update(res, gold_word, valid_rows=valid_rows)
        return res
