"""Stage-1 pre-training model: the visual frontend and a transformer encoder trained on word classification with a
second, 2-way language head (the reference's VSR_visual_frontend_pretraining_on_LRW_LRW1000_classify/, "CLS/" below).
Its frontend (and, with checkpoint.load_checkpoint's prefix_map, its encoder) then initialises the SBL model."""
import torch.nn as nn

from ._env import ops
from .video_frontend import visual_frontend

IGNORE_INDEX = -100          # nn.CrossEntropyLoss's default ignore_index (CLS/train.py:81)


class ClassifierTransformer(nn.Module):
    """CLS/transformer/transformer.py:Transformer(encoder_v, pt): frontend -> encoder_v -> fc_1500 (word) and fc_2
    (language).  Unlike the SBL Transformer, construction re-draws nothing: the layers keep their own initialisation, as in
    the reference."""

    # dp.FlatModel layout: gradient segments in the order backward completes them, and the module whose output gradient
    # marks each segment as complete (dp.GradientExchange)
    FLAT_SEGMENTS = ("fc_", "encoder_v.", "visual_frontend.resnet18.layer4.", "visual_frontend.resnet18.layer3.",
                     "visual_frontend.resnet18.layer2.", "visual_frontend.")
    FLAT_FEEDS = (("encoder_v", "fc_"), ("visual_frontend", "encoder_v."))

    def __init__(self, encoder_v, pt):
        super(ClassifierTransformer, self).__init__()
        self.visual_frontend = visual_frontend(pt)
        self.encoder_v = encoder_v
        self.fc_1500 = nn.Linear(512, 1500)
        self.fc_2 = nn.Linear(512, 2)

    def forward(self, padded_input_visual):
        """padded_input_visual (N, T, H, W), or an ops.RawClips of that logical shape (the 31st all-zero frame of the CLS loader
        is then a src_frame column of -1) -> (v_t (N, 1500) word logits, v_t_languages (N, 2) language logits).

        The shipped forward cannot run: it averages over the feature axis (`mean(dim=2, keepdim=True)`) and then feeds the
        resulting (N, T, 1) tensor to a 512-input Linear, which raises.  This restates its evident intent, the
        same restatement as oracle.sbl_oracle.cls_forward: the word head reads the encoder output averaged over time, the
        language head reads its last frame (the reference hard-codes row 30 of its 31-frame clips).  No frame is padded
        here: the reference's loader already delivers its 31 frames.  Every clip uses its full length."""
        if not isinstance(padded_input_visual, ops.RawClips):
            padded_input_visual = padded_input_visual.unsqueeze(1)
        feats = self.visual_frontend(padded_input_visual)        # (N, T, 512)
        lengths = [feats.size(1)] * feats.size(0)
        enc, *_ = self.encoder_v(feats, lengths)
        return ops.ClsHeadFn.apply(enc, self.fc_1500.weight, self.fc_1500.bias, self.fc_2.weight, self.fc_2.bias,
                                   enc.size(1) - 1)


def cal_cls_loss(v_t, v_lang, target, lang, lang_weight=0.1, ignore_index=IGNORE_INDEX):
    """loss = CE(v_t, target) + lang_weight * CE(v_lang, lang) (CLS/train.py:127-130), each CE a mean over the rows whose
    target is not ignore_index.  Sync-free: returns (loss, stats), both on the device, stats = float[6] = (loss sum, valid
    rows, correct predictions) of the word head, then of the language head (CLS/train.py:115-121)."""
    return ops.ClsLossFn.apply(v_t, v_lang, target, lang, float(lang_weight), int(ignore_index))


def cls_accuracy(stats):
    """(word accuracy, language accuracy) of a step from cal_cls_loss's stats: correct / valid rows per head (the
    reference divides by the batch size; the two agree when no target is ignored).  One host sync."""
    s = stats.detach().cpu().tolist()
    return (s[2] / s[1] if s[1] else float("nan")), (s[5] / s[4] if s[4] else float("nan"))
