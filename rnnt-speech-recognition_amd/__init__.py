"""MI355X-native RNN-T joint + transducer-loss engine (drop-in for the loss path of
noahchalifour/rnnt-speech-recognition: utils/loss.py + the warp-transducer op behind it)."""
from .build import LIB_PATH, build  # noqa: F401
from .joint import JointLoss, joint_logits, rnnt_joint_loss  # noqa: F401
from .model import HParams, Transducer, TimeReduction, Encoder, PredictionNetwork  # noqa: F401
from .train import TrainStep, run_evaluate, run_training, synthetic_batch, synthetic_trained_like_joint  # noqa: F401
from .decoding import greedy_decode, greedy_decode_batch, greedy_decode_batch_fn, greedy_decode_fn  # noqa: F401
from .decoding import beam_decode_batch, beam_decode_batch_fn, beam_search_batch  # noqa: F401
from .decoding import StreamingBeamDecoder, StreamingGreedyDecoder, StreamingMultiBeamDecoder, StreamingTranscriber  # noqa: F401
from .lstm import LSTMLayerFunction  # noqa: F401
from .biasing import ContextGraph  # noqa: F401
from .lm import NgramLM  # noqa: F401
from . import features, metrics, records  # noqa: F401
from .alignment import align_joint, rnnt_align, token_times, word_times  # noqa: F401
from .loss import RNNTLoss, get_loss_fn, reduced_lengths, rnnt_loss, rnnt_loss_and_grad  # noqa: F401
from .pruning import prune_joint_inputs, prune_ranges, rnnt_loss_pruned, rnnt_loss_pruned_and_grad  # noqa: F401
from .simple import rnnt_loss_simple, rnnt_loss_simple_and_grad, rnnt_loss_two_pass  # noqa: F401
from .pruned_joint import rnnt_joint_loss_pruned, rnnt_joint_loss_pruned_and_grad, rnnt_loss_two_pass_fused  # noqa: F401
from .pruned_training import PrunedJointLoss  # noqa: F401
from .tdt import (TDTGreedyJoint, TDTLoss, rnnt_loss_tdt, rnnt_loss_tdt_and_grad, tdt_greedy_decode,  # noqa: F401
                  tdt_greedy_search_batch)
from .tdt import StreamingTDTGreedyDecoder, TDTGreedyStreamJoint  # noqa: F401
from .tdt import rnnt_align_tdt, tdt_align_joint, token_end_frames  # noqa: F401
from .tdt import TDTBeamJoint, tdt_beam_search_batch  # noqa: F401
from .tdt import StreamingTDTBeamDecoder, TDTBeamStreamJoint  # noqa: F401
from .tdt_joint import TDTJointLoss, rnnt_joint_loss_tdt, rnnt_joint_loss_tdt_and_grad  # noqa: F401
from .ctc import CTCLoss, ctc_greedy_decode, ctc_loss, ctc_loss_and_grad  # noqa: F401

__all__ = ["rnnt_loss", "rnnt_loss_and_grad", "RNNTLoss", "get_loss_fn", "reduced_lengths", "rnnt_joint_loss",
           "joint_logits", "JointLoss", "build", "LIB_PATH", "rnnt_align", "align_joint", "token_times", "word_times",
           "rnnt_loss_pruned", "rnnt_loss_pruned_and_grad", "prune_ranges", "prune_joint_inputs",
           "rnnt_loss_simple", "rnnt_loss_simple_and_grad", "rnnt_loss_two_pass",
           "rnnt_joint_loss_pruned", "rnnt_joint_loss_pruned_and_grad", "rnnt_loss_two_pass_fused", "PrunedJointLoss",
           "rnnt_loss_tdt", "rnnt_loss_tdt_and_grad", "TDTLoss", "tdt_greedy_decode",
           "TDTGreedyJoint", "tdt_greedy_search_batch", "TDTGreedyStreamJoint", "StreamingTDTGreedyDecoder",
           "rnnt_align_tdt", "tdt_align_joint", "token_end_frames", "TDTBeamJoint", "tdt_beam_search_batch",
           "rnnt_joint_loss_tdt", "rnnt_joint_loss_tdt_and_grad", "TDTJointLoss",
           "TDTBeamStreamJoint", "StreamingTDTBeamDecoder",
           "ctc_loss", "ctc_loss_and_grad", "CTCLoss", "ctc_greedy_decode"]
