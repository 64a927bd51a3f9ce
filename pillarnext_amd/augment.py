"""GT-database paste and the four global augmentations on the device (csrc/augment.hip).

The reference does both per sample on the host (det3d/datasets/base.py:72-99): DataBaseSamplerV2.sample_all picks objects of the classes a frame
lacks, keeps those that collide with nothing, removes the scene points inside them and prepends theirs (sample_ops.py, box_np_ops.py), and
Rotation / Scaling / Translation / Flip (pipelines/augmentation.py) move the cloud and the boxes.  Here the host only chooses: which candidates
to offer (BatchSampler, the same np.random consumption) and which parameters to apply (the same draws).  Every box and every point is handled
by the kernels, between SweepMerger and the reader for the points, in front of AssignLabel for the boxes, without a device-to-host copy.

Exactness: see include/pnx.h ("Exactness contract").  Out of scope, each refused with a ValueError: gt_drop_percentage other than 0 (no
reference config uses it), database infos that carry `rot_transform`, and object points that already live on the device (reading the
database's .pkl / .bin files stays host code; the bank is uploaded once)."""
import os
import pickle

import numpy as np

from . import _lib


# ------------------------------------------------------------------------------------------------------------- the four transforms (draws only)
class Rotation:
    def __init__(self, rotation):
        self.rotation = rotation

    def draw(self):
        return float(np.random.uniform(self.rotation[0], self.rotation[1]))


class Scaling:
    def __init__(self, scale):
        self.min_scale, self.max_scale = scale

    def draw(self):
        return float(np.random.uniform(self.min_scale, self.max_scale))


class Translation:
    def __init__(self, noise):
        self.noise = noise

    def draw(self):
        return float(np.random.normal(0, self.noise, 1)[0])   # ONE scalar, later added to x, y and z alike


class Flip:
    def __init__(self, flip_prob):
        self.flip_prob = flip_prob
        if not (0 <= flip_prob[0] < 1 and 0 <= flip_prob[1] < 1):
            raise ValueError(f"flip_prob {flip_prob}: both probabilities must lie in [0, 1)")

    def draw(self):
        """(flip x, flip y): one draw per axis whose probability is > 0, x first."""
        on = [False, False]
        for axis in (0, 1):
            p = self.flip_prob[axis]
            if p > 0:
                on[axis] = bool(np.random.choice([False, True], replace=False, p=[1 - p, p]))
        return on[0], on[1]


def draw_xform(augmentations):
    """One frame's six doubles (include/pnx.h: xform) from the stages of `augmentations` (a dict or a list), drawn in its order.  The kernels
    apply rotation, scaling, translation, flip in that fixed order, which is the order of every reference config."""
    stages = list(augmentations.values()) if isinstance(augmentations, dict) else list(augmentations or [])
    a, scale, t, flags = 0.0, 1.0, 0.0, 0
    seen = []
    for st in stages:
        if isinstance(st, Rotation):
            a, flags, kind = st.draw(), flags | _lib.PNX_AUG_ROTATE, 0
        elif isinstance(st, Scaling):
            scale, flags, kind = st.draw(), flags | _lib.PNX_AUG_SCALE, 1
        elif isinstance(st, Translation):
            t, flags, kind = st.draw(), flags | _lib.PNX_AUG_TRANSLATE, 2
        elif isinstance(st, Flip):
            fx, fy = st.draw()
            flags, kind = flags | (_lib.PNX_AUG_FLIP_X if fx else 0) | (_lib.PNX_AUG_FLIP_Y if fy else 0), 3
        else:
            raise ValueError(f"{type(st).__name__} is not one of Rotation, Scaling, Translation, Flip")
        seen.append(kind)
    if seen != sorted(set(seen)):
        raise ValueError("the kernels apply rotation, scaling, translation, flip in this order, each at most once; list the stages accordingly")
    return np.array([np.cos(a), np.sin(a), a, float(np.float32(scale)), t, float(flags)], np.float64)


# ------------------------------------------------------------------------------------------------------------------------------- the sampler
class BatchSampler:
    """A shuffled index list walked in slices; a request that reaches the end returns what is left and reshuffles (sample_ops.py:10-43)."""

    def __init__(self, sampled_list, name=None, epoch=None, shuffle=True, drop_reminder=False):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx, self._example_num, self._name, self._shuffle = 0, len(sampled_list), name, shuffle

    def sample_indices(self, num):
        if self._idx + num >= self._example_num:
            ret = self._indices[self._idx:].copy()
            if self._shuffle:
                np.random.shuffle(self._indices)
            self._idx = 0
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def sample(self, num):
        return [self._sampled_list[i] for i in self.sample_indices(num)]


class DBFilterByMinNumPoint:
    def __init__(self, min_gt_point_dict, logger=None):
        self._min_gt_point_dict = min_gt_point_dict

    def __call__(self, db_infos):
        for name, min_num in self._min_gt_point_dict.items():
            if min_num > 0:
                db_infos[name] = [info for info in db_infos[name] if info["num_points_in_gt"] >= min_num]
        return db_infos


def sampled_num(rate, max_num, count):
    """round(rate * (max - count of that name among gt_names)), numpy's rounding (half to even), as sample_ops.py:123-127."""
    return int(np.round(rate * int(max_num - count)).astype(np.int64))


class DataBaseSamplerV2:
    """The reference's constructor keys, plus `db_infos` (in-memory infos {name: [info, ..]}, each info carrying its `points` (r, point_dim) fp32
    relative to the box centre; without it the infos are unpickled from root_path / dbinfo_path and each object's points are read from
    root_path / info["path"] when the bank is built) and `class_names` (the detector's class list: the class index of a pasted box is the
    position of its name there; default: the sampled classes in group order)."""

    def __init__(self, root_path=None, dbinfo_path=None, groups=(), db_prepor=None, rate=1.0, gt_drop_percentage=0, gt_drop_max_keep_points=0,
                 point_dim=5, db_infos=None, class_names=None):
        if gt_drop_percentage != 0:
            raise ValueError("gt_drop_percentage other than 0 is out of scope (no reference config uses it)")
        self.root_path, self._rate, self._point_dim = root_path, rate, int(point_dim)
        if db_infos is None:
            with open(os.path.join(str(root_path), str(dbinfo_path)), "rb") as f:
                db_infos = pickle.load(f)
        if db_prepor is not None:
            for prepor in db_prepor.values():
                db_infos = prepor(db_infos)
        self.db_infos = db_infos
        self._sample_classes, self._sample_max_nums = [], []
        for group_info in groups:
            self._sample_classes += list(group_info.keys())
            self._sample_max_nums += list(group_info.values())
        if len(self._sample_classes) > 64:
            raise ValueError("at most 64 sampled classes")
        self.class_names = list(class_names) if class_names is not None else list(self._sample_classes)
        for name, infos in db_infos.items():
            for info in infos:
                if "rot_transform" in info:
                    raise ValueError(f"a database info of class {name} carries rot_transform: out of scope")
                pts = info.get("points")
                if pts is not None and not isinstance(pts, np.ndarray):
                    raise ValueError("object points must be host numpy arrays: loading the database stays host code, the bank is uploaded once")
        self._sampler_dict = {k: BatchSampler(v, k) for k, v in db_infos.items()}   # one shuffle per class, in the dict's order
        self._bank_first, n = {}, 0
        for name in self._sample_classes:
            self._bank_first[name] = n
            n += len(db_infos[name])
        self.n_obj = n
        self._bank = {}
        self._rows = None

    @property
    def n_groups(self):
        return len(self._sample_classes)

    def _object_points(self, info):
        pts = info.get("points")
        if pts is None:
            pts = np.fromfile(os.path.join(str(self.root_path), str(info["path"])), dtype=np.float32)
        return np.asarray(pts, np.float32).reshape(-1, self._point_dim)

    def bank_host(self):
        """(points (P, point_dim) fp32, offsets (n_obj + 1) int64): the objects of the sampled classes, class by class in group order."""
        if self._rows is None:
            parts = [self._object_points(info) for name in self._sample_classes for info in self.db_infos[name]]
            off = np.zeros(len(parts) + 1, np.int64)
            off[1:] = np.cumsum([len(p) for p in parts])
            self._rows = (np.concatenate(parts, 0) if parts else np.zeros((0, self._point_dim), np.float32), off)
        return self._rows

    def bank(self, device):
        """The object bank on `device`, uploaded on first use."""
        import torch

        key = str(device)
        if key not in self._bank:
            pts, off = self.bank_host()
            self._bank[key] = (torch.from_numpy(pts).to(device), torch.from_numpy(off).to(device))
        return self._bank[key]

    def sample_frame(self, gt_classes):
        """gt_classes: the class indices (positions in class_names) of one frame's gt objects.  Returns the candidates in group order as a list of
        (bank id, box fp32, class index, group)."""
        gt_classes = np.asarray(gt_classes).reshape(-1)
        out = []
        for g, (name, max_num) in enumerate(zip(self._sample_classes, self._sample_max_nums)):
            cls = self.class_names.index(name) if name in self.class_names else -1
            num = sampled_num(self._rate, max_num, int((gt_classes == cls).sum()) if cls >= 0 else 0)
            if num > 0:
                for i in self._sampler_dict[name].sample_indices(num):
                    out.append((self._bank_first[name] + int(i), np.asarray(self.db_infos[name][int(i)]["box3d_lidar"], np.float32), cls, g))
        return out


# ------------------------------------------------------------------------------------------------------------------------------ the stage
class PasteAugment:
    """paste_and_augment with its buffers: one object per (sampler, augmentations) pair, buffers cached per batch size as AssignLabel's are."""

    def __init__(self, sampler=None, augmentations=None):
        from . import ops

        self.sampler, self.augmentations = sampler, augmentations
        self._cache = {}
        self._points = {}
        self._ws = ops.Workspace()
        self.last = None   # the buffers of the last call: accept, paste_offset, pasted_rows, frame_rows, .. (for tools and tests; all on the device)

    def _buffers(self, B, K, S, D, device):
        import torch

        key = (B, K, S, D, str(device))
        if key not in self._cache:
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
            self._cache[key] = {"accept": e((B, S), torch.uint8), "paste_offset": e((B, S), torch.int32), "boxes": e((B, K + S, D), torch.float32),
                                "classes": e((B, K + S), torch.int32), "num": e((B,), torch.int32), "pasted_rows": e((B,), torch.int32),
                                "n_out": e((1,), torch.int32), "frame_rows": e((B,), torch.int32)}
        return self._cache[key]

    def _point_buffers(self, B, capacity, width, n_points, device):
        import torch

        from . import ops

        key = (B, width, str(device))
        out = self._points.get(key)
        if out is None or out.shape[0] < capacity:
            out = self._points[key] = torch.empty((int(capacity * 1.25) + 64, width), dtype=torch.float32, device=device)
        return out[:capacity], self._ws.get(ops.paste_augment_workspace_bytes(n_points, B), device)

    def __call__(self, points, gt_boxes, gt_classes, num_gt=None, host_classes=None):
        """points (N, 1 + F) fp32 CUDA rows [batch index, x, y, z, ..] (rows with a batch index outside [0, B) are dropped: SweepMerger's output
        can be passed whole); gt_boxes (B, K, 7 or 9) fp32 CUDA; gt_classes (B, K) int32 CUDA; num_gt (B) int32 CUDA or None (= K).
        host_classes: with a sampler, the class indices of every frame's gt objects as B host arrays -- the number of candidates per class
        follows from them, and the annotations come from the host anyway; reading them back from the device would be a sync.
        Returns (points_out (capacity, 1 + F), n_out (1) int32, boxes (B, K + S, D), classes (B, K + S) int32, num (B) int32): device tensors
        of this object's cache, overwritten by the next call of the same shape.  Rows [n_out, capacity) of points_out carry batch index -1."""
        import torch

        from . import ops

        ops._need_cuda(points, "points")
        ops._need_cuda(gt_boxes, "gt_boxes")
        B, K, D = (int(v) for v in gt_boxes.shape)
        dev = gt_boxes.device
        if B > _lib.PNX_PASTE_MAX_BATCH:
            raise ValueError(f"at most {_lib.PNX_PASTE_MAX_BATCH} frames per call")
        frames = []
        xf = np.zeros((B, 6), np.float64)
        if self.sampler is not None and (host_classes is None or len(host_classes) != B):
            raise ValueError("with a sampler, host_classes must list the gt class indices of each of the B frames (host arrays)")
        for b in range(B):   # frame-major draws: the frame's candidates first (the paste runs first), then its augmentations in their order
            frames.append(self.sampler.sample_frame(host_classes[b]) if self.sampler is not None else [])
            if self.augmentations:
                xf[b] = draw_xform(self.augmentations)
        S = max(len(f) for f in frames)
        cand, bank_pts, bank_off, cand_rows = None, None, None, 0
        if S > 0:
            S = (S + 7) // 8 * 8    # few distinct shapes, few cached buffer sets
            if K + S > _lib.PNX_PASTE_MAX_BOXES:
                raise ValueError(f"{K} gt slots + {S} candidates per frame exceed {_lib.PNX_PASTE_MAX_BOXES}")
            ints = np.full((3, B, S), -1, np.int32)
            cboxes = np.zeros((B, S, D), np.float32)
            _, off = self.sampler.bank_host()
            for b, f in enumerate(frames):
                for i, (bank_id, box, cls, g) in enumerate(f):
                    if box.shape[0] != D:
                        raise ValueError(f"database boxes have {box.shape[0]} columns, the gt boxes {D}")
                    ints[0, b, i], ints[1, b, i], ints[2, b, i], cboxes[b, i] = bank_id, cls, g, box
                    cand_rows += int(off[bank_id + 1] - off[bank_id])
            ints_d = torch.from_numpy(ints).pin_memory().to(dev, non_blocking=True)
            cand = {"bank": ints_d[0], "cls": ints_d[1], "group": ints_d[2], "boxes": torch.from_numpy(cboxes).pin_memory().to(dev, non_blocking=True)}
            bank_pts, bank_off = self.sampler.bank(dev)
        xf_d = torch.from_numpy(xf).pin_memory().to(dev, non_blocking=True) if self.augmentations else None
        buf = self.last = self._buffers(B, K, S, D, dev)
        if K + S > 0:
            ops.paste_select(gt_boxes, gt_classes, num_gt, cand, bank_off, self.sampler.n_groups if cand is not None else 0, buf)
            if xf_d is not None:
                ops.augment_boxes_(buf["boxes"], buf["num"], xf_d)
        else:
            buf["num"].zero_()
        N = int(points.shape[0])
        out, ws = self._point_buffers(B, N + cand_rows, int(points.shape[1]), N, dev)
        ops.paste_augment_points(points, B, cand, buf["paste_offset"] if cand is not None else None, buf["pasted_rows"] if cand is not None else None,
                                 bank_pts, bank_off, xf_d, out, buf["n_out"], buf["frame_rows"], ws)
        return out, buf["n_out"], buf["boxes"], buf["classes"], buf["num"]


_STAGES = {}


def paste_and_augment(points, gt_boxes, gt_classes, num_gt, sampler=None, augmentations=None, host_classes=None):
    """The whole stage in one call (see PasteAugment.__call__); the buffers live in a PasteAugment kept per (sampler, augmentations) pair."""
    key = (id(sampler), id(augmentations))
    if key not in _STAGES or _STAGES[key].sampler is not sampler or _STAGES[key].augmentations is not augmentations:
        _STAGES[key] = PasteAugment(sampler, augmentations)
    return _STAGES[key](points, gt_boxes, gt_classes, num_gt, host_classes=host_classes)
