"""The device-side graph of MACnet.build (model.py:774-824) from the stem to the logits, with the
question encoder's outputs as inputs:

    images --stem--> knowledgeBase --MACCell x netLength--> memory --outputOp/classifier--> logits

`MACNetCore` takes the question encoder's outputs (vecQuestions / questionCntxWords / questionLengths) as inputs;
`MACNet` adds `embeddingsOp` + `encoder` (model.py:208-307) in front, so its inputs are exactly
the reference's feed dict: question word ids, question lengths, image features, (answers).  Every stem option set the
reference builds is covered (stem.Stem for the default CNN, stem.GenericStem for the others; the knowledge base then has
stem.out_hw cells, e.g. 7 x 7 for --stemStrideSizes 2 1).  Out of this graph stays only the host side (preprocess.py / main.py)."""
import torch

from .cell import MACCell
from .encoder import QuestionEncoder, RecurrentQuestionEncoder
from .options import UnsupportedOptions, freeze, fresh_seed, get
from .output import OutputClassifier, answer_loss_and_pred
from .params import MACCellParams
from .features import check_store_images
from .stem import Stem, check_image_index, check_image_lengths, kb_gather


class MACNetCore(torch.nn.Module):
    def __init__(self, config, H=14, W=14, imageInDim=1024, answerWordsNum=28, generator=None):
        super().__init__()
        self.config = config
        self.netLength = int(get(config, "netLength"))
        self.stem = Stem(config, H=H, W=W, inDim=imageInDim, generator=generator)
        try:
            freeze(config)
            self.cell = MACCellParams(config, self.netLength, generator=generator)
        except UnsupportedOptions:
            # an option set of the generic path (the reference's default configuration among them).  The option set and the
            # net length are known here, so the plan is compiled now and every variable it names is created now, in the plan's
            # (= TensorFlow's creation) order: tensors(), the optimizer's layout and a checkpoint load (missing / extra / shape
            # checks of checkpoint.load_reference) see exactly the variables the cell will use -- nothing is adopted by scope and
            # nothing is drawn at random behind a loaded checkpoint's back on the first forward pass
            from . import plan as _plan
            from .generic import GenericParams
            self.cell = GenericParams(generator=generator)
            for name, spec in _plan.compile_cell(config, self.netLength).variables.items():
                self.cell.ensure(name, spec.shape, spec.init)
        self.out = OutputClassifier(config, answerWordsNum=answerWordsNum, generator=generator)

    def tensors(self):
        return self.stem.tensors() + self.cell.tensors() + self.out.tensors()

    def forward(self, images, vecQuestions, questionCntxWords, questionLengths, train=False, seed=None, b0=0,
                questionWords=None, mask_word=None, image_index=None, check_index=False, kb_lengths=None,
                check_kb_lengths=False, image_lengths=None, image_ids=None):
        """Auxiliary losses: after the call `self.last_cell` is the cell of this pass.  Its attentions["kb" | "question" | "self" |
        "gate"][i], controls and memories carry the autograd edge (train / grad enabled), so a loss such as
        CE + lam * (net.last_cell.attentions["kb"][i] * target).sum() trains the stem, the encoder and the cell; infos is a constant.
        image_lengths: None, or a [G] integer device tensor for a batch whose questions share images (it needs image_index; passing
        kb_lengths as well is a ValueError): image g's knowledge base is the first image_lengths[g] of the stem's N cells.  The gather
        (macx_kb_gather_l) writes +0 into every question's padded rows, whatever the stem computed there, and makes the per-question
        kb_lengths the cell receives on the device: nothing is indexed on the host, so a captured graph follows rewritten lengths.
        check_kb_lengths=True tests 1 <= image_lengths <= N on the host first, as for kb_lengths.
        kb_lengths: None, or a [B] integer device tensor, ALWAYS per question: question b's knowledge base is the first
        kb_lengths[b] of the stem's N output cells (MACCell's kb_lengths: object features padded to a common N, grids of mixed
        sizes).  With image_index the caller passes lengths_per_image[image_index].  check_kb_lengths=True tests
        1 <= kb_lengths <= N on the host first (synchronises) and raises ValueError; unchecked values are clamped by the kernel.
        mask_word: None, or one 1-element int32 device tensor (MACCell's mask_word) handed to the stem, the cell and the output
        unit: every dropout site of the tower XORs it into its key when the kernels run (graph.CapturedTowerTrainStep).  Fused
        modules only.
        image_index: None (one image per question), or a [B] integer tensor for a batch whose questions share images: `images`
        then holds the G distinct images, question b looks at images[image_index[b]], the stem runs once per image and its output
        is gathered into the cell's [B, N, d] knowledge base (macx_kb_gather; gradients flow back through macx_kb_gather_bwd).
        With train=True the stem must not drop (stemDropout = 1.0): the reference draws that mask per question.  An index outside
        [0, G) gives that question a NaN knowledge base; check_index=True tests the range on the host first (synchronises).
        image_ids: None, or -- when `images` is a macx.FeatureStore (features resident in device memory) -- the table rows of this
        batch's images: a [B] integer device tensor, or [G] together with image_index [B].  The stem runs on
        images.gather(image_ids) (macx_features_gather; no gradient) and everything downstream is the call on that tensor.  A row
        outside [0, rows) gives that image NaN features; check_index=True tests the range on the host first.  image_ids with a
        tensor `images` is a TypeError, a store whose (H, W, C) is not the stem's a ValueError."""
        cfg = self.config
        store_ids = check_store_images(images, image_ids, self.stem, vecQuestions.shape[0] if image_index is None else None,
                                       host_check=check_index)
        per_image = images if store_ids is None else store_ids        # (what the image count is read from)
        image_index = check_image_index(image_index, vecQuestions.shape[0], train, self.stem, per_image, host_check=check_index)
        if image_lengths is not None:
            check_image_lengths(image_lengths, image_index, kb_lengths, per_image, self.stem.out_hw[0] * self.stem.out_hw[1],
                                host_check=check_kb_lengths)
        if mask_word is not None and not isinstance(self.cell, MACCellParams):
            raise UnsupportedOptions("a run's mask word over the whole tower needs the fused cell (MACCellParams); this option set "
                                     "runs the cell on the generic path")
        if questionWords is None:
            if not get(cfg, "controlContextual"):
                # mac_cell.py:570 would select the raw word embeddings; silently attending over the encoder outputs instead
                # would diverge from the reference
                raise UnsupportedOptions("without --controlContextual the cell attends over the raw word embeddings "
                                         "(mac_cell.py:570): pass them as questionWords=[B,S,ctrlDim]")
            questionWords = questionCntxWords
        seed = fresh_seed(seed, train)
        word = {} if mask_word is None else {"mask_word": mask_word}               # (None: the modules' calls of before)
        if store_ids is not None:
            images = images.gather(store_ids)                                        # macx_features_gather: [G, H*W, C] fp32
        kb = self.stem(images, train=train, seed=seed, b0=b0, **word)               # model.py:791
        if image_lengths is not None:
            kb, kb_lengths = kb_gather(kb, image_index.to(kb.device), image_lengths.to(kb.device))
            check_kb_lengths = False                                                 # (clamped by the gather; the host check is done)
        elif image_index is not None:
            kb = kb_gather(kb, image_index.to(kb.device))
        batch = images.shape[0] if image_index is None else vecQuestions.shape[0]
        lens = {} if kb_lengths is None else {"kb_lengths": kb_lengths}             # (None: the cell's call of before)
        if kb_lengths is not None:
            if check_kb_lengths and torch.is_tensor(kb_lengths) and kb_lengths.numel():
                lo, hi = int(kb_lengths.min()), int(kb_lengths.max())
                if lo < 1 or hi > kb.shape[1]:
                    raise ValueError("kb_lengths must lie in [1, %d] (the knowledge base's cells); got %d .. %d" % (kb.shape[1], lo, hi))
        cell = MACCell(vecQuestions=vecQuestions, questionWords=questionWords, questionCntxWords=questionCntxWords,
                       questionLengths=questionLengths, knowledgeBase=kb, memoryDropout=get(cfg, "memoryDropout"),
                       readDropout=get(cfg, "readDropout"), writeDropout=get(cfg, "writeDropout"), batchSize=batch,
                       train=train, config=cfg, params=self.cell, netLength=self.netLength, seed=seed, b0=b0, **word, **lens)
        state = cell.run()                                                           # model.py:801 (MACnetwork)
        self.last_cell = cell
        return self.out(state.memory, vecQuestions, train=train, seed=seed, b0=b0, **word)   # model.py:805-809

    @staticmethod
    def loss_and_pred(logits, answers, weights=None, totals=None):
        """weights / totals: output.answer_loss_and_pred's (per-question device weights with the weighted-mean loss, an
        output.AnswerTotals the launch adds to); both None is the call of before"""
        if weights is None and totals is None:
            return answer_loss_and_pred(logits, answers)                             # model.py:812-813
        return answer_loss_and_pred(logits, answers, weights=weights, totals=totals)


class MACNet(MACNetCore):
    """MACnet.build's tower body (model.py:781-813): embeddingsOp -> encoder -> stem -> MACnetwork -> outputOp/classifier.
    encoder: None -- QuestionEncoder(config) (the fused bidirectional LSTM, GenericQuestionEncoder for the other LSTM option sets);
    "recurrent" -- a RecurrentQuestionEncoder (encType RNN | GRU | LSTM, one direction or two, fused); or a module instance with
    QuestionEncoder's interface, taken as it is."""

    def __init__(self, config, vocab, H=14, W=14, imageInDim=1024, answerWordsNum=28, embInit=None, generator=None, encoder=None):
        super().__init__(config, H=H, W=W, imageInDim=imageInDim, answerWordsNum=answerWordsNum, generator=generator)
        if encoder is None:
            self.enc = QuestionEncoder(config, vocab, embInit=embInit, generator=generator)
        elif encoder == "recurrent":
            self.enc = RecurrentQuestionEncoder(config, vocab, embInit=embInit, generator=generator)
        elif isinstance(encoder, torch.nn.Module):
            self.enc = encoder
        else:
            raise ValueError('encoder must be None, "recurrent" or a module (got %r)' % (encoder,))

    def tensors(self):
        return self.enc.tensors() + super().tensors()

    def forward(self, images, questions, questionLengths, train=False, seed=None, b0=0, check_ids=True, mask_word=None,
                image_index=None, check_index=False, kb_lengths=None, image_lengths=None, image_ids=None):
        """image_ids: MACNetCore.forward's (`images` is a macx.FeatureStore and the batch names table rows); check_ids=True or
        check_index=True also tests 0 <= image_ids < rows on the host.
        image_lengths: MACNetCore.forward's (live knowledge-base cells per IMAGE of a batch with image_index).
        image_index / check_index: MACNetCore.forward's (questions that share images: `images` is [G, ...], image_index [B]).
        kb_lengths: MACNetCore.forward's (live knowledge-base cells per question); check_ids=True also tests its range on the host."""
        store_ids = check_store_images(images, image_ids, self.stem, questions.shape[0] if image_index is None else None,
                                       host_check=check_ids or check_index)
        per_image = images if store_ids is None else store_ids
        check_image_index(image_index, questions.shape[0], train, self.stem, per_image, host_check=check_index)
        if image_lengths is not None:
            check_image_lengths(image_lengths, image_index, kb_lengths, per_image, self.stem.out_hw[0] * self.stem.out_hw[1],
                                host_check=check_ids)
        seed = fresh_seed(seed, train)
        word = {} if mask_word is None else {"mask_word": mask_word}
        words, vecQ = self.enc(questions, questionLengths, train=train, seed=seed, b0=b0, check_ids=check_ids, **word)   # model.py:783-788
        raw = None
        if not get(self.config, "controlContextual"):
            # mac_cell.py:570: the control unit attends over the embedded words themselves (embeddingsOp's output, no dropout)
            raw = self.enc.embed(questions)
            if raw.shape[-1] != get(self.config, "ctrlDim"):
                raise ValueError("Dimensions must be equal: without --controlContextual the question words are wrdEmbDim = %d wide, "
                                 "the control state ctrlDim = %d (mac_cell.py:154)" % (raw.shape[-1], get(self.config, "ctrlDim")))
        return super().forward(images, vecQ, words, questionLengths, train=train, seed=seed, b0=b0, questionWords=raw,
                               image_index=image_index, kb_lengths=kb_lengths, check_kb_lengths=check_ids and image_lengths is None, **word,
                               **({} if image_lengths is None else {"image_lengths": image_lengths}),
                               **({} if image_ids is None else {"image_ids": image_ids}))
