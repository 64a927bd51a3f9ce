"""CPU: configs/mvf18_aspp_waymo.yaml -- the third detector family of the reference (configs/experiments/waymo_det_mvf18_aspp_iou_car.yaml over
configs/models/detectors/mvf18_aspp.yaml and configs/models/reader/mvf_encoder.yaml) -- loads, resolves and instantiates through the det3d aliases."""
import os

from conftest import ROOT


def test_mvf18_config_instantiates_a_detector_without_a_backbone():
    from pillarnext_amd import config
    from pillarnext_amd.models import ASPPNeck, CenterHead, SingleStageDetector
    from pillarnext_amd.mvf_encoder import MVFFeatureNet
    from pillarnext_amd.voxel_encoder import grid_of

    cfg = config.load(os.path.join(ROOT, "configs", "mvf18_aspp_waymo.yaml"))
    m = cfg["model"]
    assert "backbone" not in m and m["_target_"] == "det3d.models.detectors.single_stage.SingleStageDetector"
    r = m["reader"]
    assert r["_target_"] == "det3d.models.readers.mvf_encoder.MVFFeatureNet"
    assert {k: v for k, v in r.items() if k != "_target_"} == dict(
        in_channels=5, voxel_size=[0.075, 0.075, 20], pc_range=[-76.8, -76.8, -10.0, 76.8, 76.8, 10.0], cylinder_range=[-180, -10.0, 0, 180, 10.0, 107],
        cylinder_size=[0.140625, 0.2, 107], num_filters=[48, 48], layer_nums=[2, 2, 2, 2], ds_layer_strides=[1, 2, 2, 2], ds_num_filters=[48, 96, 192, 192],
        kernel_size=[3, 3, 3, 3], out_channels=256)
    # the interpolations resolve to the reader's geometry and the shared task / stride lists
    for blk in ("head", "post_processing"):
        assert m[blk]["voxel_size"] == r["voxel_size"] and m[blk]["pc_range"] == r["pc_range"] and m[blk]["out_size_factor"] == [4, 4], blk
    assert m["head"]["tasks"] == [["vehicle"], ["pedestrian", "cyclist"]] and m["head"]["rectifier"] == [[0.68], [0.71, 0.65]]
    assert m["head"]["common_heads"]["iou"] == [1, 2] and m["head"]["with_reg_iou"] is True and m["head"]["weight"] == 1
    assert m["post_processing"]["nms"] == dict(nms_pre_max_size=4096, nms_post_max_size=500, nms_iou_threshold=[[0.7], [0.2, 0.25]])
    assert m["neck"]["in_channels"] == 256 and not any("${" in str(v) for v in (m["head"], m["post_processing"]))

    det = config.instantiate(m)
    assert isinstance(det, SingleStageDetector) and det.backbone is None
    assert isinstance(det.reader, MVFFeatureNet) and isinstance(det.neck, ASPPNeck) and isinstance(det.head, CenterHead)
    sd = det.state_dict()
    assert tuple(sd["reader.pillarview.blocks.0.0.conv.weight"].shape) == (48, 48, 3, 3)
    assert tuple(sd["reader.cylinderview.blocks.3.0.conv.weight"].shape) == (192, 192, 3, 3)
    assert tuple(sd["reader.pillarview.pfn_layers.0.linear.weight"].shape) == (24, 20)        # a non-last PFN layer halves its width: 48 / 2
    assert tuple(sd["reader.pointnet1.linear.weight"].shape) == (192, 20)
    assert tuple(sd["reader.pointnet2.linear.weight"].shape) == (256, 3 * 192)
    assert [s[0].norm.num_features for s in det.reader.pillarview.blocks] == [48, 96, 192, 192]
    assert [len(s) for s in det.reader.cylinderview.blocks] == [3, 3, 3, 3]
    iou = [k for k in sd if k.startswith("head.tasks.1.iou.")]
    assert iou and tuple(sd[[k for k in iou if k.endswith("weight")][-1]].shape)[0] == 1      # one IoU channel per task
    assert tuple(sd[[k for k in sd if k.startswith("head.tasks.1.hm.") and k.endswith("weight")][-1]].shape)[0] == 2
    # the pillar grid is 2048 x 2048, the reader's map grid / 8 and the head map grid / 4 (the head's stride-2 deblock)
    g = grid_of(r["pc_range"], r["voxel_size"])
    assert (int(g[0]), int(g[1])) == (2048, 2048) and int(det.reader.ds_rate) == 8
    assert tuple(int(v) for v in grid_of(r["cylinder_range"], r["cylinder_size"])[:2]) == (2560, 100)
    assert m["head"]["strides"] == [2, 2] and 2048 // int(det.reader.ds_rate) * 2 == 2048 // m["head"]["out_size_factor"][0] == 512
