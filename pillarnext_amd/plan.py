"""Launch tables for include/pnx.h::pnx_enqueue: the C-ABI calls of a model section with their arguments frozen once, replayed per frame
batch by ONE call (csrc/enqueue.hip).  A builder method takes what the wrapper of the same call in ops.py takes and passes that wrapper's
own argument checks (the helpers in front of it there), but records the call instead of issuing it; tensors named as `dynamic` are re-bound per step (bind),
everything else must stay alive and in place -- the plan keeps references."""
import ctypes

from . import ops
from ._lib import PnxError, check, lib, stream_ptr

OP_MASK_POOL3, OP_TILE_LIST, OP_CONV3X3, OP_DECONV2X2, OP_SEPHEAD_OUT = 1, 2, 3, 4, 5


class PnxOp(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("i", ctypes.c_int32 * 9), ("p", ctypes.c_void_p * 11)]


assert ctypes.sizeof(PnxOp) == 128, "pnx_op layout drifted (include/pnx.h)"


class Dyn:
    """A tensor argument that changes from step to step: `like` gives the shape / dtype / layout every bound tensor must have."""

    def __init__(self, name, like):
        self.name, self.like = name, like


class LaunchPlan:
    def __init__(self):
        self._ops, self._keep, self._dyn, self._arr = [], [], {}, None

    def __len__(self):
        return len(self._ops)

    def _add(self, kind, ints, ptrs):
        if self._arr is not None:
            raise PnxError("the plan is frozen")
        op = PnxOp()
        op.kind = kind
        for k, v in enumerate(ints):
            op.i[k] = int(v)
        for k, a in enumerate(ptrs):
            if isinstance(a, Dyn):    # bound per step: only the description of the tensor is kept
                meta = (a.like.shape, a.like.dtype, a.like.stride(), a.like.device)
                self._dyn.setdefault(a.name, (meta, []))[1].append((len(self._ops), k))
                op.p[k] = a.like.data_ptr()
            elif a is not None:
                op.p[k] = a.data_ptr()
                self._keep.append(a)
        self._ops.append(op)

    # ---- builders (ops.py: mask_pool3, conv_tile_list, conv3x3_masked, deconv2x2, sephead_out); each returns what its call will write.
    # dt (PNX_BF16 / PNX_F16) selects the pnx_*_f16 twin in csrc/enqueue.hip
    def mask_pool3(self, mask_in, mask_out, stride):
        self._add(OP_MASK_POOL3, [*ops._like(mask_in).shape, stride], [mask_in, ops.mask_pool3_out(mask_in, stride, mask_out)])
        return mask_out

    def tile_list(self, mask, dirties, tile_rows, out):
        if len(dirties) > 8:
            raise PnxError("tile_list: an entry has room for 8 row_dirty arrays")
        tl, tc = ops.conv_tile_buffers(mask, tile_rows, out)
        self._add(OP_TILE_LIST, [len(dirties), *ops._like(mask).shape, tile_rows], [mask, tl, tc] + list(dirties))
        return out

    def conv3x3(self, x, wfrag, bias, cout, stride=1, mask=None, residual=None, relu=True, out=None, tiles=None):
        """out = (y, row_dirty) workspace pair, or (y, None) for a plain output buffer."""
        B, H, W, ci, dt, _, _ = ops._conv3x3_dims(x, wfrag, cout, stride, mask, residual, out)
        tl, tc = tiles if tiles is not None else (None, None)
        self._add(OP_CONV3X3, [B, H, W, ci, cout, stride, 1 if relu else 0, dt], [x, wfrag, bias, residual, mask, *out, tl, tc])
        return out[0]

    def deconv2x2(self, x, wfrag, bias, cout, y, relu=True):
        B, H, W, ci, dt = ops._conv_dims("deconv2x2", x, wfrag, y, cout, 2)
        self._add(OP_DECONV2X2, [B, H, W, ci, cout, 1 if relu else 0, dt], [x, wfrag, bias, y])
        return y

    def sephead_out(self, x, wfrag, bias, y):
        B, H, W, ci, dt = ops._conv_dims("sephead_out", x, wfrag, y, 16, 1)
        self._add(OP_SEPHEAD_OUT, [B, H, W, ci // 64, dt], [x, wfrag, bias, y])
        return y

    # ---- replay
    def freeze(self):
        self._arr = (PnxOp * max(len(self._ops), 1))(*self._ops)   # copies: the entries of the array are what bind() patches
        self._bound = {}
        return self

    def bind(self, name, t):
        if self._arr is None:
            self.freeze()
        meta, where = self._dyn[name]
        if (t.shape, t.dtype, t.stride(), t.device) != meta:
            raise PnxError(f"plan: tensor bound to '{name}' differs from the one the plan was built for")
        a = t.data_ptr()
        for k, j in where:
            self._arr[k].p[j] = a
        self._bound[name] = t   # alive until the next binding: the launches read / write it asynchronously

    def run(self):
        if self._arr is None:
            self.freeze()
        missing = set(self._dyn) - set(self._bound)
        if missing:   # an unbound slot would replay the build-time pointer, which nothing keeps alive
            raise PnxError(f"plan: dynamic tensors never bound: {sorted(missing)}")
        if not all(a.is_cuda for a in self._keep) or not all(t.is_cuda for t in self._bound.values()):
            raise PnxError("plan: every tensor of a launch table must live on the GPU")   # the library has no CPU path
        check(lib().pnx_enqueue(self._arr, len(self._ops), stream_ptr()), "pnx_enqueue")
