"""AssignLabel on the device: ground-truth boxes -> the per-task label lists CenterHead.loss reads.

The reference's det3d/datasets/pipelines/assign.py:5-116 is a pipeline stage on the host: a Python loop over the objects of one frame that
draws numpy Gaussian patches, after which the loader uploads the dense heat maps (4.5 MB per nuScenes frame).  This class keeps the
reference's constructor keys (configs/dataset/base/base_det_train.yaml plus the experiment's tasks / pc_range / voxel_size /
out_size_factor) and does the work of a whole frame batch in one call of csrc/assign.hip."""
import numpy as np

from . import _lib


class AssignLabel:
    def __init__(self, tasks, gaussian_overlap, max_objs, min_radius, pc_range, voxel_size, out_size_factor):
        self.tasks = [list(t) for t in tasks]
        self.gaussian_overlap, self.max_objs, self.min_radius = float(gaussian_overlap), int(max_objs), int(min_radius)
        self.pc_range = np.asarray(pc_range, np.float64)
        self.voxel_size = np.asarray(voxel_size, np.float64)
        T = len(self.tasks)
        osf = np.asarray(out_size_factor, np.int64).reshape(-1)
        self.out_size_factor = [int(v) for v in (np.repeat(osf, T) if osf.size == 1 else osf)]
        if len(self.out_size_factor) != T:
            raise ValueError(f"{len(self.out_size_factor)} out_size_factor entries for {T} tasks")
        # assign.py:32-34,41: grid = round((hi - lo) / voxel) in fp64, feature map = grid[:2] // out_size_factor
        self.grid = np.round((self.pc_range[3:] - self.pc_range[:3]) / self.voxel_size).astype(np.int64)
        self.map_size = [(int(self.grid[1] // f), int(self.grid[0] // f)) for f in self.out_size_factor]   # (H, W) per task
        self.class_names = [n for t in self.tasks for n in t]
        self.class_table = [(ti, ni) for ti, t in enumerate(self.tasks) for ni in range(len(t))]             # global class -> (task, class in task)
        if T < 1 or T > _lib.PNX_ASSIGN_MAX_TASKS or len(self.class_names) > _lib.PNX_ASSIGN_MAX_CLASSES:
            raise ValueError(f"AssignLabel is built for 1..{_lib.PNX_ASSIGN_MAX_TASKS} tasks and up to {_lib.PNX_ASSIGN_MAX_CLASSES} classes")
        self._name_to_index = {}
        for i, n in enumerate(self.class_names):
            self._name_to_index[n] = i           # a name listed twice: the last entry wins, as in the reference's dict (assign.py:26-29)
        self._cache = {}

    def descriptor(self):
        d = _lib.PnxAssignDesc()
        d.lo[0], d.lo[1] = float(self.pc_range[0]), float(self.pc_range[1])
        d.voxel[0], d.voxel[1] = float(self.voxel_size[0]), float(self.voxel_size[1])
        d.overlap, d.min_radius, d.max_objs = self.gaussian_overlap, self.min_radius, self.max_objs
        d.n_tasks, d.n_classes = len(self.tasks), len(self.class_table)
        for t, names in enumerate(self.tasks):
            d.osf[t], d.h[t], d.w[t], d.ncls[t] = self.out_size_factor[t], self.map_size[t][0], self.map_size[t][1], len(names)
        for g, (ti, ni) in enumerate(self.class_table):
            d.class_task[g], d.class_cls[g] = ti, ni
        return d

    def class_index(self, names):
        """Global class index of every name (int32 numpy array), -1 for a name no task lists (the reference skips those objects)."""
        return np.asarray([self._name_to_index.get(n, -1) for n in names], np.int32)

    def _buffers(self, B, device):
        import torch

        from . import ops

        key = (B, str(device))
        if key not in self._cache:
            M, T = self.max_objs, len(self.tasks)
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
            out = {"hm": [e((B, len(t), *self.map_size[i]), torch.float32) for i, t in enumerate(self.tasks)],
                   "anno_box": [e((B, M, 10), torch.float32) for _ in range(T)], "ind": [e((B, M), torch.int64) for _ in range(T)],
                   "mask": [e((B, M), torch.uint8) for _ in range(T)], "cat": [e((B, M), torch.int64) for _ in range(T)],
                   "gt_boxes": [e((B, M, 7), torch.float32) for _ in range(T)]}
            counts = e((B, T), torch.int32)
            ws = e((ops.assign_workspace_bytes(B, T, M),), torch.uint8)
            self._cache[key] = (out, counts, ws, self.descriptor())
        return self._cache[key]

    def assign(self, gt_boxes, gt_classes, num_gt=None):
        """gt_boxes (B, K, 9) fp32 CUDA [x y z dx dy dz vx vy yaw], gt_classes (B, K) int32 CUDA (class_index values), num_gt (B) int32 CUDA
        or None (= K objects in every frame).  Returns {hm, anno_box, ind, mask, cat, gt_boxes: one tensor per task, counts: (B, tasks) int32}.
        The tensors are this object's cached buffers for the batch size: the next call with the same B overwrites them."""
        from . import ops

        ops._need_cuda(gt_boxes, "gt_boxes")
        out, counts, ws, desc = self._buffers(int(gt_boxes.shape[0]), gt_boxes.device)
        ops.assign_labels(gt_boxes, gt_classes, num_gt, desc, out, counts, ws)
        res = {k: list(v) for k, v in out.items()}
        res["counts"] = counts
        return res
