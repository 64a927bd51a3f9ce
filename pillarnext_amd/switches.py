"""The Python-side environment switches, in one table.  on(NAME) reads the environment at the moment it is called: unset = the default, "1" = on,
"0" = off, anything else is an error; a name that is not in the table is a KeyError, so a misspelt switch cannot silently select the default.
Not here: what the C library reads itself (getenv under csrc/), the build's switches (build.py), PNX_LIB (_lib.py) and bench.py's PNX_BENCH_*."""
import os

from ._lib import PnxError

# name: (default, meaning)
SWITCHES = {
    # read on every call -- tests flip them between two runs of one model
    "PNX_MASKED_BN_HIP": (True, "the masked BatchNorm + residual + ReLU node on csrc/masked_bn.hip; off: its torch statement"),
    "PNX_TRAIN_HIPCONV": (True, "bf16-autocast training: 3x3 layers on the masked HIP kernels; off: MIOpen"),
    "PNX_TRAIN_HIPWGRAD": (True, "bf16-autocast training: weight gradient on csrc/conv_wgrad.hip; off: MIOpen's dense wrw"),
    "PNX_TRAIN_F32_HIP": (True, "fp32 training: 3x3 layers as bf16 pieces on the masked HIP kernels; off: MIOpen fp32"),
    "PNX_TRAIN_DENSE_HIP": (True, "bf16-autocast training: the neck's and the head's dense 3x3 layers on the masked kernels; off: MIOpen"),
    "PNX_TRAIN_DENSE_BN_HIP": (True, "training: dense BatchNorm2d [+ ReLU] of the neck and the head on the masked BatchNorm node; off: the modules"),
    "PNX_TRAIN_HEAD_HIP": (True, "training: the SepHead output convolutions (64 -> k <= 4) on csrc/head_train.hip; off: MIOpen"),
    "PNX_TRAIN_HIP_DGRAD_S2": (True, "training: stride-2 data gradient on csrc/conv_dgrad_s2.h; off: MIOpen / CK"),
    "PNX_FUSED_LOSS": (True, "CenterHead.loss on csrc/center_loss.hip; off: the torch losses of losses.py"),
    "PNX_TRAIN_FUSED": (True, "the reader's fused training passes (pfn_train.py); off: torch Linear / BatchNorm1d + HIP scatter-max"),
    "PNX_TRAIN_BILINEAR_HIP": (True, "multi-view reader, training: point sampling on pnx_bilinear_gather[_backward]; off: the torch statement"),
    "PNX_TRAIN_POINT_HIP": (False, "multi-view reader, training: Linear + BatchNorm1d + ReLU [+ per-cell max] of the PFN layers and the PointNets on "
                                   "csrc/point_layer_train.hip; off: the torch modules"),
    "PNX_HEAD_LAZY_TORCH": (False, "lazy head: evaluate the candidates with the torch statement of the kernel's arithmetic"),
    # read once, when a FusedPillarNeXt is built
    "PNX_HIP_CONV": (True, "fused graph: 3x3 layers, deblock and head output on the HIP kernels; off: MIOpen + one epilogue pass"),
    "PNX_PLAN": (True, "fused graph: the backbone and the head as one launch plan each; off: every launch issued from Python"),
    "PNX_SPARSE_WS": (True, "fused graph: persistent stage workspaces that touch only active or stale row segments"),
    "PNX_TILE_LISTS": (True, "fused graph: one list of active tiles per stage for its stride-1 convolutions"),
    "PNX_DECODE_STREAM": (True, "fused graph: the decoder on its own stream, behind the next batch's reader"),
    "PNX_HEAD_LAZY": (True, "fused graph: regression branches evaluated at the decoder's candidates only"),
    # read once, when a PackedDecoder is built
    "PNX_DECODE_TOPK": (True, "decoder: radix-select top-k candidate selection (pre_max <= 4096); off: a full sort"),
    "PNX_DECODE_TORCH_SORT": (False, "decoder without top-k: torch.sort instead of the key-sort kernels"),
    # not a bool: 2 or 3, read by train_f32_pieces() below at every forward of the fp32 node
    "PNX_TRAIN_F32_PIECES": (2, "fp32 training: bf16 pieces per operand, 2 = three products, 3 = six products (fp32-accurate)"),
}

_DEFAULT = {name: default for name, (default, _) in SWITCHES.items() if isinstance(default, bool)}


def on(name):
    """Is the switch on?  One dict lookup and one os.environ.get: it is called some hundreds of times per training step."""
    default = _DEFAULT[name]
    v = os.environ.get(name)
    if v is None:
        return default
    if v == "1":
        return True
    if v == "0":
        return False
    raise PnxError(f"{name} must be unset (default {'1' if default else '0'}), 0 or 1; got {v!r}")


def train_f32_pieces():
    """bf16 pieces per fp32 operand in the fp32 graph's 3x3 layers (PNX_TRAIN_F32_PIECES): 2 (default) = the three-product node, 3 = the six-product
    form (fp32-accurate; ~2x the MFMA work of those layers).  Anything else is an error."""
    v = os.environ.get("PNX_TRAIN_F32_PIECES", "2").strip()
    if v not in ("2", "3"):
        raise PnxError(f"PNX_TRAIN_F32_PIECES must be 2 or 3, got {v!r}")
    return int(v)
