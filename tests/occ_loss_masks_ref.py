"""What tests/test_occ_loss_masks_cpu.py and tests/test_gpu_occ_loss_masks.py share: the reference's lines for the sample
masks of loss_occ's train_cfg variants restated literally (ococc_bbox_head.py:706-710, 713-722, 730-734, 749-753, 792;
the [M, K, D] feature repeats and the decoder left out: the ori logits are an input), and the crafted edge inputs."""
import numpy as np
import torch

FLAG_SUBSETS = [(o, b, u) for o in (False, True) for b in (False, True) for u in (False, True)]


def reference_lines(occ_smp_xyz, pred_box_size, occ_label_scores, ori_occ_preds, occ_labels, occ_label_thresh, pos_thresh,
                    no_loss_for_outside, no_loss_for_observed_feats, residual_loss):
    """occ_smp_xyz [M, K, 3], pred_box_size [M, 3], occ_label_scores [M], ori_occ_preds [M, K, 1] (or None),
    occ_labels [M, K] int64 (1: occupied) -> (occ_weights [M * K], unmatched_mask [M * K] bool or None, the three
    counts as Python ints)."""
    M, K = occ_labels.shape
    get_cls_from_pred = lambda pred: (pred.sigmoid() > pos_thresh).long().squeeze(-1)   # occ_base.py, cls_dim 1
    occ_weights = torch.zeros_like(occ_label_scores)
    occ_weights[occ_label_scores > occ_label_thresh] = 1
    occ_weights = occ_weights.view(M, 1).repeat(1, K)
    if no_loss_for_outside:
        occ_smp_mask = (occ_smp_xyz >= -pred_box_size[:, None, :] / 2).all(dim=-1) & (
            occ_smp_xyz <= pred_box_size[:, None, :] / 2).all(dim=-1)
        occ_weights = occ_weights * occ_smp_mask.float()
    if no_loss_for_observed_feats:
        ori_pred_cls = get_cls_from_pred(ori_occ_preds)
        unobserved_mask = ori_pred_cls == 0
        occ_weights = occ_weights * unobserved_mask.float()
    unmatched_mask = None
    if residual_loss:
        ori_pred_cls = get_cls_from_pred(ori_occ_preds).view(-1)
        unmatched_mask = occ_labels.view(-1) != ori_pred_cls
    valid_mask = occ_weights.view(-1) > 0
    counts = [int(valid_mask.sum()), int(unmatched_mask.sum()) if residual_loss else 0,
              int((unmatched_mask & valid_mask).sum()) if residual_loss else 0]
    return occ_weights.view(-1), unmatched_mask, counts


EDGE_LOGITS = [0.0, 1e-8, -1e-8, 6e-8, -6e-8, 1.2e-7, -1.2e-7, 1e-6, -1e-6, 88.0, -88.0, float('inf'), float('-inf'),
               float('nan')]


def edge_case(device='cpu'):
    """3 RoIs x 42 samples: every edge logit under both label values, in RoIs whose label score is above, equal to
    (weight 0) and above the threshold; coordinates exactly on +-size / 2 (inside), one ulp beyond (outside), NaN
    (outside) on each axis in turn, the other axes well inside.  -> dict(xyz, box_size, score, score_thresh, ori_logits,
    labels), every tensor on ``device``."""
    size = np.array([[1.9, 4.7, 1.6], [2.1, 5.3, 1.7], [0.3, 0.7, 1e-3]], np.float32)
    half = size / np.float32(2)
    M = 3
    coords = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for kind in ('on', 'beyond', 'nan'):
                coords.append((axis, sign, kind))
    K = 42
    logits = (EDGE_LOGITS * 3)[:K]
    xyz = np.zeros((M, K, 3), np.float32)
    labels = np.zeros((M, K), np.int64)
    for i in range(M):
        for k in range(K):
            p = (half[i] * np.float32(0.25)).copy()
            axis, sign, kind = coords[k % len(coords)]
            edge = np.float32(sign) * half[i, axis]
            if kind == 'beyond':
                edge = np.nextafter(edge, np.float32(sign * np.inf), dtype=np.float32)
            elif kind == 'nan':
                edge = np.float32('nan')
            if k < 2 * len(coords):
                p[axis] = edge
            xyz[i, k] = p
            labels[i, k] = (k // 7 + i) % 2 if k % 5 else 2    # (a label that is neither 0 nor 1 is "not occupied")
    T = lambda a: torch.from_numpy(a).to(device)
    return dict(xyz=T(xyz), box_size=T(size), score=T(np.array([0.9, 0.4, 0.41], np.float32)), score_thresh=0.4,
                ori_logits=T(np.tile(np.array(logits, np.float32), (M, 1))), labels=T(labels))
