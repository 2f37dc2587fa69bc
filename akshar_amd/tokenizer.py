"""Drop-in `aksharTokenizer` (reference: src/akshar/tokenizer.py:18-288) on the MI355X engine.

Same constructor, methods, return types and errors as the reference:
  - model_path missing / not a file -> akshar-level fallback (model_type "akshar")      :67-71
  - model_type not in {"sentencepiece", "bpe"} -> ValueError("unknown model_type: ...")  :101-102
  - encode()/decode() without a model -> ValueError("need model for IDs" / "... to decode") :187-188,213-214
The per-string methods run a batch of one through the GPU; `encode_batch` / `tokenize_batch` /
`encode_packed` are the batched forms (one launch for many rows). The reference's engine
libraries (sentencepiece, tokenizers) are not used: models are read from their files
(akshar_amd.models) and run by the HIP kernels.
"""
import os
from typing import List, Optional, Union

import numpy as np

from . import decode as _dec
from . import engine
from . import longrows
from .normalize import normalize_batch
from .segment import _split, analyze_batch, composition_from, segment_batch


class aksharTokenizer:
    """High-level tokenizer for Hindi/Sanskrit/Hinglish text (tokenizer.py:18)."""

    def __init__(self, model_path: Optional[str] = None, model_type: str = "sentencepiece",
                 normalize_roman: bool = True, clean_hinglish: bool = True):
        self.model_path = model_path
        self.normalize_roman = normalize_roman
        self.clean_hinglish = clean_hinglish
        self.model = None
        self._configured_model_type = model_type
        if model_path and os.path.exists(model_path):
            self._load_model()
        else:
            self.model_type = "akshar"

    def _load_model(self):
        model_type = self._configured_model_type
        if model_type == "sentencepiece":
            self.model = engine.SPM(self.model_path)
            self.model_type = "sentencepiece"
        elif model_type == "bpe":
            self.model = engine.BPE(self.model_path)
            self.model_type = "bpe"
        else:
            raise ValueError(f"unknown model_type: {model_type}")

    @property
    def _flags(self):
        return engine.flags_of(self.normalize_roman, self.clean_hinglish)

    # ---------------------------------------------------------------- preprocessing
    def preprocess(self, text: str) -> str:
        pieces = self._long_pieces(text)
        if pieces is not None:  # a long row: its exact pieces (longrows.py), normalized as a batch
            return "".join(normalize_batch(pieces, self.normalize_roman, self.clean_hinglish))
        return normalize_batch([text], self.normalize_roman, self.clean_hinglish)[0]

    @staticmethod
    def _long_pieces(text):
        """The exact pieces of a long text (longrows.py), or None for a text kept as one row."""
        if len(text) * 4 <= longrows.LONG_ROW_BYTES:
            return None
        raw = text.encode("utf-8", "surrogatepass")
        if len(raw) <= longrows.LONG_ROW_BYTES:
            return None
        cuts = longrows.cut_points(raw)
        if len(cuts) == 0:
            return None
        b = [0] + [int(c) for c in cuts] + [len(raw)]
        return [raw[b[i]:b[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(b) - 1)]

    def preprocess_batch(self, texts: List[str]) -> List[str]:
        return normalize_batch(texts, self.normalize_roman, self.clean_hinglish)

    # ---------------------------------------------------------------- ids
    def encode_packed(self, buf, offs, nbytes=None):
        """Device rows (uint8 bytes, int64 offsets) -> device (int32 ids, int64 row offsets)."""
        if self.model is None:
            raise ValueError("need model for IDs")
        return self.model.encode_batch(buf, offs, flags=self._flags, nbytes=nbytes)

    def _encode_rows(self, texts):
        """list[str] or a (buf, offs) device pair -> device (int32 ids, int64 row offsets)."""
        if self.model is None:
            raise ValueError("need model for IDs")
        if isinstance(texts, tuple):
            return self.encode_packed(*texts)
        hb, ho = engine.pack_host(list(texts))
        buf, offs = engine.to_device(hb, ho)
        return self.encode_packed(buf, offs, nbytes=int(ho[-1]))

    def _pad_id(self, pad_id):
        pad_id = self.model.model.pad_id if pad_id is None else pad_id
        if pad_id is None:
            raise ValueError("the model has no <pad> token: pass pad_id")
        return int(pad_id)

    def encode_padded(self, texts, max_length: int, *, padding_side: str = "right", truncation_side: str = "right",
                      pad_id: Optional[int] = None) -> dict:
        """texts (list[str] or a (buf, offs) device pair) -> {"input_ids" [n, max_length],
        "attention_mask" bool, "lengths" int32 [n]} as device tensors: HF tokenizers' enable_truncation
        + enable_padding(length=max_length). BPE rows keep their <s> ... </s> through truncation (the
        template is applied after it); pad_id defaults to the model's <pad>."""
        if self.model is None:
            raise ValueError("need model for IDs")
        pad_id = self._pad_id(pad_id)
        keep = 1 if self.model_type == "bpe" else 0
        ids, oo = self._encode_rows(texts)
        out, mask, lengths = engine.pad_ids(ids, oo, max_length, pad_id, padding_side=padding_side,
                                            truncation_side=truncation_side, keep_head=keep, keep_tail=keep)
        return {"input_ids": out, "attention_mask": mask, "lengths": lengths}

    def encode_blocks(self, texts, block_size: int, *, sep_id=..., pad_id: Optional[int] = None,
                      drop_last: bool = False) -> dict:
        """texts (list[str] or a (buf, offs) device pair) -> {"input_ids" [n_blocks, block_size],
        "position_ids", "doc_ids"} as device tensors: the rows' ids concatenated and cut into blocks
        (LM pretraining's "group texts"), with each token's index inside its row and its row index so
        attention can be kept inside documents. sep_id follows every row: by default the model's </s>
        for SentencePiece and none for BPE (its rows end in </s> already); None for no separator."""
        if self.model is None:
            raise ValueError("need model for IDs")
        pad_id = self._pad_id(pad_id)
        if sep_id is ...:
            sep_id = self.model.model.eos_id if self.model_type == "sentencepiece" else None
        ids, oo = self._encode_rows(texts)
        out, pos, doc = engine.pack_ids(ids, oo, block_size, sep_id=sep_id, pad_id=pad_id, drop_last=drop_last)
        return {"input_ids": out, "position_ids": pos, "doc_ids": doc}

    def encode_windows(self, texts, max_length: int, *, stride: int = 0, text_pair=None, truncation: str = "only_second",
                       max_fixed_length: Optional[int] = None, padding_side: str = "right",
                       pad_id: Optional[int] = None) -> dict:
        """texts (and text_pair: each a list[str] or a (buf, offs) device pair) -> sliding windows of
        max_length ids as device tensors (engine.window_ids: input_ids, attention_mask, token_type_ids,
        overflow_to_sample_mapping, window_start, lengths, win_offs): HF tokenizers'
        enable_truncation(max_length, stride) with its overflow encodings kept, padded to max_length.
        With a pair, truncation names what slides: "only_second" repeats the text in front of every
        window of its text_pair (a question and its context), "only_first" slides the text in front of
        its repeated text_pair, "longest_first" (stride 0) gives one window per pair with the longer
        side cut first. The repeated side is cut to max_fixed_length ids if given (at most
        max_length - stride - 1 less the sliding side's <s> </s>, the default: larger values are
        lowered to it), so it is cut only as far as it must be to leave the other side room. BPE rows keep their <s> ... </s> in every window.
        Unlike HF, token_type_ids are 0 on the whole first segment and 1 on the whole second one."""
        if self.model is None:
            raise ValueError("need model for IDs")
        if text_pair is not None and truncation not in ("only_second", "only_first", "longest_first"):
            raise ValueError("truncation must be 'only_second', 'only_first' or 'longest_first', got %r" % (truncation,))
        pad_id = self._pad_id(pad_id)
        keep = 1 if self.model_type == "bpe" else 0
        kw = dict(stride=stride, keep_head=keep, keep_tail=keep, padding_side=padding_side)
        ids, oo = self._encode_rows(texts)
        if text_pair is None:
            return engine.window_ids(ids, oo, max_length, pad_id, **kw)
        if max_fixed_length is not None:
            if int(max_fixed_length) < 0:
                raise ValueError("max_fixed_length must not be negative")
            max_fixed_length = min(int(max_fixed_length), max(int(max_length) - 2 * keep - int(stride) - 1, 0))
        pair = self._encode_rows(text_pair)
        if truncation == "only_first":
            return engine.window_ids(ids, oo, max_length, pad_id, fixed=pair, fixed_cap=max_fixed_length, fixed_last=True, **kw)
        if truncation == "longest_first":
            return engine.window_ids(*pair, max_length, pad_id, fixed=(ids, oo), longest_first=True, **kw)
        return engine.window_ids(*pair, max_length, pad_id, fixed=(ids, oo), fixed_cap=max_fixed_length, **kw)

    def _word_start(self, dev):
        """uint8 [vocab_size] on `dev`: 1 for the SentencePiece pieces that begin with U+2581 (a word's
        first piece); built once per device and kept."""
        cache = self.__dict__.setdefault("_word_start_cache", {})
        if dev not in cache:
            import torch
            flags = np.fromiter((p.startswith(b"\xe2\x96\x81") for p in self.model.model.pieces), dtype=np.uint8,
                                count=self.model.model.vocab_size)
            cache[dev] = torch.from_numpy(flags).to(dev)
        return cache[dev]

    def encode_mlm(self, texts, max_length: int, *, mlm_probability: float = 0.15, seed: int = 0, stream_id: int = 0,
                   whole_word: bool = False, mask_fraction: float = 0.8, random_fraction: float = 0.1,
                   mask_id: Optional[int] = None, ignore_index: int = -100, padding_side: str = "right",
                   truncation_side: str = "right", pad_id: Optional[int] = None) -> dict:
        """texts (list[str] or a (buf, offs) device pair) -> {"input_ids" [n, max_length],
        "attention_mask" bool, "labels", "lengths" int32 [n]} as device tensors: encode_padded's batch
        masked for encoder pretraining (engine.mask_ids, BERT's rule): mlm_probability of the tokens
        carry a label, and of those mask_fraction show the model's <mask>, random_fraction a random id
        of the vocabulary and the rest themselves; every other label is ignore_index. Padding and the
        model's <pad> <unk> <s> </s> <mask> are never selected. The same (seed, stream_id) gives the
        same batch on every run; pass the epoch or the rank as stream_id for another draw.
        whole_word (SentencePiece only): a word's pieces are selected together, a word beginning at
        every piece that starts with U+2581. BPE ids carry no word boundaries (the Whitespace
        pre-tokenizer drops them), so whole_word raises ValueError there."""
        if self.model is None:
            raise ValueError("need model for IDs")
        m = self.model.model
        mask_id = m.mask_id if mask_id is None else mask_id
        if mask_id is None:
            raise ValueError("the model has no <mask> token: pass mask_id")
        if whole_word and self.model_type != "sentencepiece":
            raise ValueError("whole_word needs a SentencePiece model: BPE ids carry no word boundaries")
        pad_id = self._pad_id(pad_id)
        if self.model_type == "bpe":
            special = (pad_id, m.unk_token_id, m.bos, m.eos, mask_id)
        else:
            special = (pad_id, m.unk_id, m.bos_id, m.eos_id, mask_id)
        never = sorted({int(v) for v in special if v is not None})
        keep = 1 if self.model_type == "bpe" else 0
        ids, oo = self._encode_rows(texts)
        out, mask, lengths = engine.pad_ids(ids, oo, max_length, pad_id, padding_side=padding_side,
                                            truncation_side=truncation_side, keep_head=keep, keep_tail=keep)
        inputs, labels = engine.mask_ids(out, mask, mask_id=int(mask_id), vocab_range=(0, m.vocab_size), never=never,
                                         mlm_probability=mlm_probability, mask_fraction=mask_fraction,
                                         random_fraction=random_fraction, seed=seed, stream_id=stream_id,
                                         word_start=self._word_start(out.device) if whole_word else None,
                                         ignore_index=ignore_index)
        return {"input_ids": inputs, "attention_mask": mask, "labels": labels, "lengths": lengths}

    def encode_spans(self, texts, inputs_length: int, *, noise_density: float = 0.15, mean_span_length: float = 3.0,
                     sentinel_first: Optional[int] = None, sentinel_step: Optional[int] = None, seed: int = 0,
                     stream_id: int = 0, dtype=None, pad_id: Optional[int] = None) -> dict:
        """texts (list[str] or a (buf, offs) device pair) -> {"input_ids" [n_blocks, inputs_length],
        "labels" [n_blocks, label_length], "input_lengths", "label_lengths"} as device tensors:
        span-corruption batches for encoder-decoder pretraining (T5's objective, engine.span_ids). The
        rows' ids are packed (encode_blocks, its default separator, no partial last block) into blocks
        of engine.span_raw_length(inputs_length) ids, the longest whose corrupted form fits
        inputs_length, and every block is corrupted: noise_density of its ids in spans of
        mean_span_length on average; the inputs show one sentinel per span and end in </s>, the labels
        list every sentinel and its span, end in </s> and are padded with -100. By default every
        sentinel is the model's <mask> (BART's text infilling: the shipped vocabularies reserve no
        sentinel range). For T5's numbered sentinels pass sentinel_first (and sentinel_step, -1 if left
        out) of a vocabulary that reserves the ids sentinel_first, sentinel_first + sentinel_step, ...;
        ValueError if a block has more spans than ids lie between sentinel_first and the vocabulary's
        end in that direction. pad_id defaults to the model's <pad>. The same (seed, stream_id) gives
        the same batch on every run; pass the epoch or the rank as stream_id for another draw."""
        import torch
        if self.model is None:
            raise ValueError("need model for IDs")
        m = self.model.model
        n_sentinels = None
        if sentinel_first is None:
            if m.mask_id is None:
                raise ValueError("the model has no <mask> token: pass sentinel_first")
            if sentinel_step not in (None, 0):
                raise ValueError("sentinel_step needs sentinel_first: the default sentinel is <mask> for every span")
            sentinel_first, sentinel_step = m.mask_id, 0
        else:
            sentinel_first = int(sentinel_first)
            sentinel_step = -1 if sentinel_step is None else int(sentinel_step)
            if sentinel_step < 0:  # the range runs down to id 0
                n_sentinels = sentinel_first // -sentinel_step + 1 if sentinel_first >= 0 else 0
            elif sentinel_step > 0:
                n_sentinels = max(0, -(-(m.vocab_size - sentinel_first) // sentinel_step))
        eos_id = m.eos if self.model_type == "bpe" else m.eos_id
        block, _ = engine.span_raw_length(inputs_length, noise_density=noise_density, mean_span_length=mean_span_length,
                                          eos=True)
        if block < 2:
            raise ValueError("inputs_length = %d leaves no room for a span" % int(inputs_length))
        pad_id = self._pad_id(pad_id)
        ids = self.encode_blocks(texts, block, pad_id=pad_id, drop_last=True)["input_ids"]
        if dtype not in (None, torch.int32):
            ids = ids.to(dtype)
        return engine.span_ids(ids, noise_density=noise_density, mean_span_length=mean_span_length,
                               sentinel_first=sentinel_first, sentinel_step=sentinel_step, eos_id=eos_id, pad_id=pad_id,
                               in_width=int(inputs_length), seed=seed, stream_id=stream_id, n_sentinels=n_sentinels)

    def encode_batch(self, texts: List[str]) -> List[List[int]]:
        if self.model is None:
            raise ValueError("need model for IDs")
        if not texts:
            return []
        if len(texts) == 1:  # a batch of one: the single-call path (host staging, one sync)
            return [self.encode(texts[0])]
        hb, ho = engine.pack_host(texts)
        buf, offs = engine.to_device(hb, ho)
        ids, oo = self.encode_packed(buf, offs, nbytes=int(ho[-1]))
        return engine.id_lists(ids.cpu().numpy(), oo.cpu().numpy())

    def encode(self, text: str) -> List[int]:
        if self.model is None:
            raise ValueError("need model for IDs")
        if self.model_type == "bpe":
            raw = text.encode("utf-8", "surrogatepass")
            if len(raw) > longrows.LONG_ROW_BYTES and self._cuts_ok():  # one long row -> its exact pieces, stitched
                buf, offs = longrows.split_rows(raw)
                gb, go = engine.to_device(buf, offs)
                ids, oo = self.encode_packed(gb, go, nbytes=len(raw))
                return [int(x) for x in longrows.stitch_bpe(ids.cpu().numpy(), oo.cpu().numpy())]
            return self.model.encode_host(raw, self._flags).tolist()
        # SentencePiece: always one row (its lattice carries a float score across the whole row).
        # One string: the per-call path (one kernel for a row that fits a tile, else host staging)
        return self.model.encode_host(text.encode("utf-8", "surrogatepass"), self._flags).tolist()

    def _cuts_ok(self):
        """No added token spans a long-row cut point (' ' or '\n' inside one)."""
        return not any(" " in c or "\n" in c for c, _ in self.model.model.added)

    def decode(self, ids: List[int]) -> str:
        """tokenizer.py:195-219, on the device (ak_bpe_decode / ak_spm_decode)."""
        return self.decode_batch([ids])[0]

    def decode_batch(self, rows: List[List[int]]) -> List[str]:
        if self.model is None:
            raise ValueError("need model to decode")
        return engine.decode_lists(self.model, [list(r) for r in rows])

    # ---------------------------------------------------------------- tokens
    def _tokens_for(self, ids):
        if self.model_type == "sentencepiece":
            return _dec.spm_pieces(self.model.model, ids)
        return _dec.bpe_tokens(self.model.model, ids)

    def tokenize_batch(self, texts: List[str], return_metadata: bool = False):
        if not return_metadata:
            if self.model is None:
                norms = self.preprocess_batch(texts)
                return [_split(n, e) for n, e in zip(norms, segment_batch(norms))]
            return [self._tokens_for(ids) for ids in self.encode_batch(texts)]
        # normalize + segment + script runs of every text in one fused pass (ak_analyze)
        norms, ends, runs = analyze_batch(texts, self._flags)
        if self.model is None:
            toks = [_split(n, e) for n, e in zip(norms, ends)]
        else:
            toks = [self._tokens_for(ids) for ids in self.encode_batch(texts)]
        metas = [composition_from(n, len(e), r) for n, e, r in zip(norms, ends, runs)]
        out = []
        for text, norm, meta, t in zip(texts, norms, metas, toks):
            meta = dict(meta)
            meta["tokens"] = t
            meta["token_count"] = len(t)
            meta["original_text"] = text
            meta["normalized_text"] = norm
            out.append(meta)
        return out

    def tokenize(self, text: str, return_metadata: bool = False) -> Union[List[str], dict]:
        if not return_metadata:
            if self.model is None:
                pieces = self._long_pieces(text)
                if pieces is not None:  # clusters of the exact pieces (longrows.py), concatenated
                    norms = self.preprocess_batch(pieces)
                    return [t for n, e in zip(norms, segment_batch(norms)) for t in _split(n, e)]
            else:
                return self._tokens_for(self.encode(text))
        return self.tokenize_batch([text], return_metadata)[0]

    def detokenize(self, tokens: List[str]) -> str:
        """tokenizer.py:221-246 (pure string handling, unchanged)."""
        if self.model_type == "sentencepiece":
            txt = "".join(tokens)
            txt = txt.replace("▁", " ")
            return txt.strip()
        elif self.model_type == "bpe":
            txt = " ".join(tokens)
            txt = txt.replace(" ##", "")
            txt = txt.replace("Ġ", " ")
            return txt.strip()
        return "".join(tokens)

    # ---------------------------------------------------------------- analysis
    def explain(self, text: str) -> dict:
        (norm,), (ends,), (runs,) = analyze_batch([text], self._flags)  # one fused pass
        akshars = _split(norm, ends)
        switches = list(zip(_split(norm, [e for e, _ in runs]), [lab for _, lab in runs]))
        stats = composition_from(norm, len(ends), runs)
        tokens = self.tokenize(text)
        return {"original": text, "normalized": norm, "akshars": akshars, "code_switches": switches,
                "tokens": tokens, "stats": stats}

    def vocab_size(self) -> int:
        if self.model is None:
            return 0
        return self.model.model.vocab_size


AksharTokenizer = aksharTokenizer
Akshar = aksharTokenizer
