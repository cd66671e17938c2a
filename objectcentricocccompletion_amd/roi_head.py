"""TrackletRoIHeadOCC / TrackletDetectorOCC -- host mirror of
mmdet3d/models/roi_heads/tracklet_roi_head_occ.py (forward_train :85-114, simple_test
:492-610, test_occ :394-486, _bbox_forward(_train) :759-878, _assign_and_sample :880-991,
_select_one2one_candidates :993-1030, tracklets2rois :1045-1060, get_gt_rois :1065-1075) and
mmdet3d/models/detectors/tracklet_detector_occ.py (:96-198, :313-345).  Same type strings,
constructor arguments, loss-dict keys and result-dict keys; tracklets are the plain-tensor
``Tracklet`` of tracklet.py."""
import os

import torch
from torch import nn

from ._lib import const_tensor
from .bbox import points_box_to_box, rotation_3d_in_axis
from .occ import occ_ops
from .occ.layers import TemporalCache
from .registry import BBOX_ASSIGNERS, DETECTORS, HEADS, ROI_EXTRACTORS
from .tracklet import SamplingResult, Tracklet


BATCHED_ASSIGN = os.environ.get('OCOCC_BATCHED_ASSIGN', '1') == '1'   # assignment / sampling of all tracklets at once
# test_occ's per-RoI occupancy counts: one HIP launch per chunk, counts kept on the device (0: the ATen chain and a
# read-back per chunk, occ_iou_counts_aten -- also what the CPU stand-ins of oracle/cpu_port.py run)
OCC_IOU_KERNEL = os.environ.get('OCOCC_OCC_IOU_KERNEL', '1') != '0'


def bbox3d2roi(bbox_list):
    """[N_i, 7] per sample -> [sum N_i, 8] with the sample index in column 0."""
    # (the sample index column for the whole list at once: the per-sample fill + concatenation was three launches per
    # tracklet, ~200 of a 64-tracklet step's)
    from .tracklet import host_index
    boxes = torch.cat(list(bbox_list), 0)
    col = [float(i) for i, b in enumerate(bbox_list) for _ in range(b.size(0))]
    idx = host_index(col, boxes.device, dtype=boxes.dtype) if boxes.is_floating_point() else host_index(
        [int(v) for v in col], boxes.device, dtype=boxes.dtype)
    rois = torch.cat([idx.view(-1, 1), boxes], dim=-1)
    # (largest sample index present + 1, known from the list's shapes: what the head would otherwise read back from
    # column 0 -- ococc_bbox_head.py:851 ``int(rois_batch_idx.max().item() + 1)``)
    rois._ococc_batch_size = max((i + 1 for i, b in enumerate(bbox_list) if b.size(0) > 0), default=0)
    return rois


def check_save_occ_cfg(test_cfg):
    """test_cfg.save_occ (export the completed occupancy from simple_test) needs occ_save_root and excludes test_cfg.tta:
    the augmented frames are not the frames to export.  Checked when the head is built, before any forward pass."""
    if not test_cfg or not test_cfg.get('save_occ', False):
        return
    if test_cfg.get('tta', None) is not None:
        raise ValueError('test_cfg.save_occ with test_cfg.tta: the augmented frames are not the frames to export')
    if not test_cfg.get('occ_save_root', None):
        raise ValueError('test_cfg.save_occ needs test_cfg.occ_save_root, the directory the files go to')


def check_save_gt_occ_cfg(test_cfg):
    """test_cfg.save_gt_occ (export the annotated occupancy, cropped to the proposals, from simple_test) needs
    gt_occ_save_root and excludes test_cfg.tta, as check_save_occ_cfg."""
    if not test_cfg or not test_cfg.get('save_gt_occ', False):
        return
    if test_cfg.get('tta', None) is not None:
        raise ValueError('test_cfg.save_gt_occ with test_cfg.tta: the augmented frames are not the frames to export')
    if not test_cfg.get('gt_occ_save_root', None):
        raise ValueError('test_cfg.save_gt_occ needs test_cfg.gt_occ_save_root, the directory the files go to')


class OnlineState(object):
    """What frame-by-frame inference keeps between steps (TrackletRoIHeadOCC.online_begin): ``cache``, the TemporalCache of
    the temporal transformer, and ``frames``, the steps taken per slot (a list of ints on the host: the cache's own
    ``pos_host``, since a slot's frame index is the number of frames it has cached).  ``origin``: per slot the inverse of
    the ego pose at the slot's first step (world -> the slot's fixed frame, a float64 4x4 array on the host), kept by
    simple_test_scene_step, None for a slot that is free or was stepped through simple_test_step."""

    def __init__(self, cache):
        self.cache = cache
        self.origin = [None] * cache.slots

    @property
    def frames(self):
        return self.cache.pos_host

    @property
    def slots(self):
        return self.cache.slots

    def reset(self, slots=None):
        self.cache.reset(slots)
        for s in (range(self.cache.slots) if slots is None else [int(s) for s in slots]):
            self.origin[s] = None


@HEADS.register_module()
class TrackletRoIHeadOCC(nn.Module):

    def __init__(self, num_classes=3, roi_extractor=None, bbox_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None, general_cfg=dict(), history_only=False):
        super().__init__()
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        check_save_occ_cfg(test_cfg)
        check_save_gt_occ_cfg(test_cfg)
        self.general_cfg, self.num_classes = general_cfg, num_classes
        self.with_roi_scores = general_cfg.get('with_roi_scores', False)
        self.with_roi_corners = general_cfg.get('with_roi_corners', False)
        self.roi_extractor = ROI_EXTRACTORS.build(roi_extractor)
        bh = dict(bbox_head)
        bh['train_cfg'], bh['test_cfg'] = train_cfg, test_cfg
        self.bbox_head = HEADS.build(bh)
        if train_cfg is not None:
            self.bbox_assigner = BBOX_ASSIGNERS.build(train_cfg['assigner'])
        self.history_only = history_only

    # ------------------------------------------------------------------ training
    def forward_train(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, img_metas, tracklet_list,
                      gt_candidates_list, gt_occs_list, gt_occ_scores_list):
        samples = self._assign_and_sample(tracklet_list, gt_candidates_list, gt_occs_list, gt_occ_scores_list,
                                          pts_batch_idx, pts_frame_inds)
        return dict(self._bbox_forward_train(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, samples)['loss_bbox'])

    def _select_one2one_candidates(self, tracklet_list, candidates_list, gt_occs_list, gt_occ_scores_list):
        """Per proposal tracklet: the GT candidate with most frames of IoU > candidate_thresh
        (tracklet_roi_head_occ.py:993-1030).  The reference walks tracklets and candidates and reads one count back per
        pair; here the timestamp matching of the whole batch is done on the host first, ALL (proposal box, candidate
        box) pairs go through one aligned-IoU launch, the counts come back in one read, and the per-frame IoUs of the
        chosen candidates are left with the proposals for the assigner (Tracklet.self_ious)."""
        from .tracklet import aligned_iou_3d, host_index
        cfg = self.train_cfg if self.train_cfg is not None else self.test_cfg
        thr = cfg.get('candidate_thresh', 0.5)
        dev = tracklet_list[0].device
        p_off, c_off, i1, i2, seg, spans = 0, 0, [], [], [], []   # spans[(t, c)] = (start, end, own frame indices)
        c_boxes = []
        for t, (trk, cands) in enumerate(zip(tracklet_list, candidates_list)):
            for c, cand in enumerate(cands):
                a, b = trk.common_frames(cand)
                spans.append((t, c, len(i1), len(i1) + len(a), a))
                i1 += [p_off + v for v in a]
                i2 += [c_off + v for v in b]
                seg += [len(spans) - 1] * len(a)
                c_boxes.append(cand.boxes[:, :7])
                c_off += len(cand)
            p_off += len(trk)
        counts, ious = [0] * len(spans), None
        if i1:
            P = torch.cat([t.boxes[:, :7] for t in tracklet_list], 0)
            C = torch.cat(c_boxes, 0)
            ious = aligned_iou_3d(P[host_index(i1, dev)], C[host_index(i2, dev)])
            hits = torch.zeros(len(spans), device=dev).index_add_(0, host_index(seg, dev), (ious > thr).float())
            counts = [int(v) for v in hits.tolist()]          # the one read-back of the selection
        best = {}
        for k, (t, c, lo, hi, own) in enumerate(spans):
            if t not in best or counts[k] > counts[best[t]]:   # first maximum, as torch.argmax
                best[t] = k
        out_trks, out_occs, out_scores = [], [], []
        for t, (trk, cands, occs, scores) in enumerate(zip(tracklet_list, candidates_list, gt_occs_list or [None] * len(tracklet_list),
                                                            gt_occ_scores_list or [None] * len(tracklet_list))):
            if len(cands) == 0:
                out_trks.append(trk.new_empty())
                out_occs.append(None)
                out_scores.append(None)
                continue
            _, c, lo, hi, own = spans[best[t]]
            out_trks.append(cands[c])
            out_occs.append(occs[c] if occs is not None else None)
            out_scores.append(scores[c] if scores is not None else None)
            if hi > lo and own == list(range(len(trk))):
                over = ious[lo:hi]
            else:
                over = trk.boxes.new_zeros(len(trk))
                if hi > lo:
                    over = over.index_copy(0, host_index(own, dev), ious[lo:hi])
            # valid for this candidate object and for the box tensors as they are now (in-place transforms bump _version)
            trk._self_iou_cache = (cands[c], trk.boxes, over, trk.boxes._version, cands[c].boxes._version)
        return out_trks, out_occs, out_scores

    def _assign_and_sample_batched(self, tracklet_list, gts, occs, occ_scores, pts_batch_idx, pts_frame_inds):
        """The loop below for TrackletAssigner without object_centric / keep_frame_inds, where everything but the box,
        score and IoU rows themselves follows from timestamps, i.e. is known on the host: the index lists of the whole
        batch go up in ONE copy, the rows are gathered from the concatenated tensors in one launch per field, and the
        per-tracklet SamplingResults are views of those (the reference's per-tracklet form costs ~25 launches and 3-4
        small uploads per tracklet: half of the launches of a 64-tracklet step).  Same fields, same values."""
        from .tracklet import host_index
        dev = tracklet_list[0].device
        shift_on = bool(self.train_cfg.get('random_shift_frame_inds', False))
        n_of, m_of, idx_of, pos_of, neg_of, shifts = [], [], [], [], [], []
        for trk, gt in zip(tracklet_list, gts):
            n, m = len(trk), len(gt)
            if m == 0 or n == 0:
                idx = [0 if m == 0 else -1] * n
            else:
                idx = [gt.get_index_from_ts(ts) + 1 for ts in trk.ts_list]
            n_of.append(n)
            m_of.append(m)
            idx_of.append(idx)
            pos_of.append([i for i, g in enumerate(idx) if g > 0])
            neg_of.append([i for i, g in enumerate(idx) if g == 0])
            shifts.append(int(torch.randint(0, 200 - n + 1, (1,)).item()) if shift_on else 0)   # (CPU generator)
        # global row numbers into the concatenated tensors
        big, cuts = [], []

        def part(values):
            cuts.append((len(big), len(big) + len(values)))
            big.extend(values)
            return len(cuts) - 1

        box_off, gt_off = 0, 0
        pos_g, neg_g, order_g, pos_gt_g, pos_assigned, frame_inds, labels_pos = [], [], [], [], [], [], []
        pos_loc = [i for p in pos_of for i in p]      # the indices the reference's fields hold: local to the tracklet
        neg_loc = [i for q in neg_of for i in q]
        for t, trk in enumerate(tracklet_list):
            order = pos_of[t] + neg_of[t]
            pos_g += [box_off + i for i in pos_of[t]]
            neg_g += [box_off + i for i in neg_of[t]]
            order_g += [box_off + i for i in order]
            pos_gt_g += [gt_off + idx_of[t][i] - 1 for i in pos_of[t]]
            pos_assigned += [idx_of[t][i] - 1 for i in pos_of[t]]
            frame_inds += [i + shifts[t] for i in order]
            labels_pos += [gts[t].type] * len(pos_of[t])
            box_off += n_of[t]
            gt_off += m_of[t]
        k_pos, k_neg, k_ord, k_pgt, k_pas, k_fr, k_lab, k_shift, k_ploc, k_nloc = (part(v) for v in (
            pos_g, neg_g, order_g, pos_gt_g, pos_assigned, frame_inds, labels_pos, shifts, pos_loc, neg_loc))
        up = host_index(big, dev)
        take = lambda k: up[cuts[k][0]:cuts[k][1]]
        cur_all = torch.cat([t.concated_boxes() for t in tracklet_list], 0)
        scores_all = torch.cat([t.concated_scores().detach() for t in tracklet_list], 0)
        over_all = torch.cat([trk.self_ious(gt) if (m and n) else trk.boxes.new_zeros(n)
                              for trk, gt, n, m in zip(tracklet_list, gts, n_of, m_of)], 0)
        have_gt = [gt.concated_boxes() for gt, m in zip(gts, m_of) if m > 0]
        n_pos = [len(p) for p in pos_of]
        n_neg = [len(q) for q in neg_of]
        n_ord = [a + b for a, b in zip(n_pos, n_neg)]
        pos_boxes = cur_all[take(k_pos)].split(n_pos)
        neg_boxes = cur_all[take(k_neg)].split(n_neg)
        if have_gt:
            gt_all = torch.cat(have_gt, 0)
            pos_gt_boxes = gt_all[take(k_pgt)].split(n_pos)
        iou = over_all[take(k_ord)].detach().split(n_ord)
        boxes_ord = cur_all[take(k_ord)].split(n_ord)     # (= cat(pos_bboxes, neg_bboxes) per tracklet, without the cats)
        scores = scores_all[take(k_ord)].split(n_ord)
        pos_local = take(k_ploc).split(n_pos)
        neg_local = take(k_nloc).split(n_neg)
        pas = take(k_pas).split(n_pos)
        frames = take(k_fr).split(n_ord)
        labels = take(k_lab).split(n_pos)
        if shift_on:   # the points of tracklet t move by the same shift as its boxes (one gather + one add for the batch)
            pts_frame_inds += take(k_shift)[pts_batch_idx.long()].to(pts_frame_inds.dtype)
        results = []
        for t, (trk, gt) in enumerate(zip(tracklet_list, gts)):
            s = SamplingResult.__new__(SamplingResult)
            s.pos_inds, s.neg_inds = pos_local[t], neg_local[t]
            s.pos_bboxes, s.neg_bboxes = pos_boxes[t], neg_boxes[t]
            s._bboxes = boxes_ord[t]
            s.num_gts = m_of[t]
            s.pos_assigned_gt_inds = pas[t]
            gtb = gt.concated_boxes()
            s.pos_gt_bboxes = gtb.new_zeros((0, 7)) if gtb.numel() == 0 else pos_gt_boxes[t]
            s.pos_gt_labels = labels[t]
            s.iou, s.scores, s.bboxes_frame_inds = iou[t], scores[t], frames[t]
            s.occ_labels, s.occ_scores = occs[t], occ_scores[t]
            results.append(s)
        return results

    def _assign_and_sample(self, tracklet_list, candidates_list, gt_occs_list, gt_occ_scores_list, pts_batch_idx,
                           pts_frame_inds):
        gts, occs, occ_scores = self._select_one2one_candidates(tracklet_list, candidates_list, gt_occs_list,
                                                                gt_occ_scores_list)
        from .tracklet import TrackletAssigner
        if (BATCHED_ASSIGN and type(self.bbox_assigner) is TrackletAssigner and not self.bbox_assigner.object_centric
                and not self.train_cfg.get('keep_frame_inds', True) and all(len(t) > 0 for t in tracklet_list)):
            return self._assign_and_sample_batched(tracklet_list, gts, occs, occ_scores, pts_batch_idx, pts_frame_inds)
        results = []
        for tid, (trk, gt) in enumerate(zip(tracklet_list, gts)):
            cur = trk.concated_boxes()
            assign = self.bbox_assigner.assign(trk, gt)
            s = SamplingResult(assign, cur, gt.concated_boxes())
            order = torch.cat([s.pos_inds, s.neg_inds])
            s.iou = assign.max_overlaps[order].detach()
            n = len(cur)
            base = torch.arange(n, device=trk.device, dtype=torch.long)
            if self.train_cfg.get('keep_frame_inds', True):
                fr = torch.unique(pts_frame_inds[pts_batch_idx == tid])
                if len(fr) < n:
                    fr = torch.cat([fr, fr[-1:].repeat(n - len(fr))])
                s.bboxes_frame_inds = fr[order]
            elif self.train_cfg.get('random_shift_frame_inds', False):
                shift = int(torch.randint(0, 200 - n + 1, (1,)).item())
                pts_frame_inds[pts_batch_idx == tid] += shift
                s.bboxes_frame_inds = base[order] + shift
            else:
                s.bboxes_frame_inds = base[order]
            s.scores = assign.scores[order]
            s.occ_labels, s.occ_scores = occs[tid], occ_scores[tid]
            results.append(s)
        return results

    def _bbox_forward_train(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, sampling_results):
        rois = bbox3d2roi([r.bboxes for r in sampling_results])
        roi_frame_inds = torch.cat([r.bboxes_frame_inds for r in sampling_results])
        roi_scores = torch.cat([r.scores for r in sampling_results])
        res = self._bbox_forward(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, roi_scores, roi_frame_inds)
        pre = self.train_cfg.get('transform_occ_pre', False)
        targets = self.bbox_head.get_targets(sampling_results, self.train_cfg, transform_occ=pre,
                                             num_occ_per_tracklet=self.train_cfg.get('num_occ_per_tracklet', -1))
        loss = self.bbox_head.loss(res, rois, *targets, transform_occ=not pre, roi_frame_inds=roi_frame_inds)
        labels = targets[0].view(-1) > 0.5
        preds = res['cls_score'].view(-1).sigmoid().detach() > 0.5
        # four of the reference's five logging figures (tracklet_roi_head_occ.py:803-824) from ONE reduction: the counts are sums of
        # 0 / 1 in f32 (exact), so every figure has the value its own float().sum() chain gives -- in a dozen launches
        # instead of three dozen
        hit, miss = preds & labels, ~(preds | labels)
        c = torch.stack([hit, preds, labels, miss, ~preds, ~labels]).float().sum(1)
        # (index tensors from the constant cache: a Python list as an index is a pageable host-to-device copy = a host sync)
        num, den = const_tensor((0, 0, 3, 3), c.device, torch.long), const_tensor((1, 2, 4, 5), c.device, torch.long)
        ratios = c[num] / (c[den] + 1e-6)
        loss['acc'] = (preds == labels).float().mean().detach()
        (loss['precision_posbox'], loss['recall_posbox'], loss['precision_negbox'], loss['recall_negbox']) = ratios.unbind(0)
        res.update(loss_bbox=loss)
        return res

    def _bbox_forward(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, roi_scores, roi_frame_inds):
        """Pool the points of every RoI, append the RoI score, run the head (:828-878)."""
        pooled = self._pool_points(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, roi_scores, roi_frame_inds)
        return self.bbox_head(*pooled, rois, roi_frame_inds)

    def _pool_points(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, roi_scores, roi_frame_inds):
        """The points of every RoI with the RoI score / corner offsets appended: (xyz, features, pooling info, RoI index)."""
        assert pts_xyz.size(0) == pts_feats.size(0) == pts_batch_idx.size(0) == pts_frame_inds.size(0)
        inds, roi_inds, info = self.roi_extractor(pts_xyz[:, :3], pts_batch_idx, pts_frame_inds, rois[:, :8],
                                                  roi_frame_inds)
        new_feats, new_xyz = pts_feats[inds], pts_xyz[inds]
        if self.with_roi_scores:
            new_feats = torch.cat([new_feats, roi_scores[roi_inds].unsqueeze(1)], 1)
        if self.with_roi_corners:
            new_feats = torch.cat([new_feats, self.roi_corner_offsets(rois, roi_inds, new_xyz).to(new_feats.dtype)], 1)
        return new_xyz, new_feats, info, roi_inds

    @staticmethod
    def roi_corner_offsets(rois, roi_inds, xyz):
        """27 extra point features of general_cfg.with_roi_corners (tracklet_roi_head_occ.py:861-868): the offsets from
        the point to the 8 corners of its RoI and to a ninth "centre" row, over 10.  The reference takes that ninth row
        from the first three RoI COLUMNS, (batch index, x, y) -- reproduced as is (tests/golden/roi_corners.npz)."""
        from .bbox import box_corners
        c = torch.cat([box_corners(rois[:, 1:]).to(xyz.dtype), rois[:, :3].to(xyz.dtype)[:, None, :]], 1)   # [R, 9, 3]
        return (c[roi_inds.long()] - xyz[:, None, :]).reshape(xyz.size(0), 27) / 10

    # ------------------------------------------------------------------ inference
    def tracklets2rois(self, tracklets):
        rois = bbox3d2roi([t.concated_boxes()[:, :7] for t in tracklets])
        frames = torch.cat([torch.arange(len(t), device=rois.device, dtype=torch.long) for t in tracklets])
        return rois, frames, torch.cat([t.concated_scores() for t in tracklets]), \
            torch.cat([t.concated_labels() for t in tracklets])

    def get_gt_rois(self, tracklets, gt_tracklets):
        boxes, masks = zip(*[gt.concated_boxes_from_ts(trk.ts_list) for trk, gt in zip(tracklets, gt_tracklets)])
        return torch.cat([torch.cat(masks, 0)[:, None].float(), torch.cat(boxes, 0)], 1)

    def simple_test(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, img_metas, tracklet_list,
                    gt_candidates_list=None, gt_occs_list=None, gt_occ_scores_list=None, **kwargs):
        """One tracklet at a time (batch size 1, as the reference asserts): ``[dict(out_tracklets=[refined
        tracklet], inters, unions, gt_boxes)]`` (tracklet_roi_head_occ.py:492-610).  The refined tracklet is a
        copy of the proposal updated through Tracklet.update_from_prediction (RoIs without points keep their
        proposal box and score); with test_occ_iou the per-RoI occupancy intersection / union counts follow."""
        assert len(tracklet_list) == 1, 'only support batch size 1'
        if self.test_cfg.get('online', False):   # (this package's key: frame by frame over a K/V cache, the same result)
            return self.simple_test_online(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, img_metas, tracklet_list,
                                           gt_candidates_list, gt_occs_list, gt_occ_scores_list)
        gt_rois, gt_occ_list, gt_occ_score_list = self._test_gt_rois(tracklet_list, gt_candidates_list, gt_occs_list,
                                                                     gt_occ_scores_list)
        rois, roi_frame_inds, cls_preds, labels_3d = self.tracklets2rois(tracklet_list)
        res = self._bbox_forward(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, cls_preds, roi_frame_inds)
        decoded = self.bbox_head.get_bboxes_from_tracklet(rois, res['cls_score'], res['bbox_pred'],
                                                          res['nonempty_roi_mask'], labels_3d, cls_preds, img_metas,
                                                          gt_rois=gt_rois, cfg=self.test_cfg)
        return self._test_results(tracklet_list, decoded, res, rois, roi_frame_inds, img_metas, gt_rois, gt_occ_list,
                                  gt_occ_score_list, pts_xyz, pts_batch_idx, pts_frame_inds)

    def _test_gt_rois(self, tracklet_list, gt_candidates_list, gt_occs_list, gt_occ_scores_list):
        """(GT boxes aligned to the proposal [R, 8] with the matched flag first, occupancy labels, their scores) of the
        candidate selected for the tracklet; three Nones without candidates"""
        if gt_candidates_list is None:
            return None, None, None
        gts, gt_occ_list, gt_occ_score_list = self._select_one2one_candidates(
            tracklet_list, gt_candidates_list, gt_occs_list, gt_occ_scores_list)
        return self.get_gt_rois(tracklet_list, gts), gt_occ_list, gt_occ_score_list

    def _test_results(self, tracklet_list, decoded, res, rois, roi_frame_inds, img_metas, gt_rois, gt_occ_list,
                      gt_occ_score_list, pts_xyz, pts_batch_idx, pts_frame_inds):
        """simple_test behind the head: the refined tracklet, the occupancy counts, the exports"""
        out_tracklets = []
        for i, trk in enumerate(tracklet_list):
            new = trk.clone()
            boxes, scores, labels, valid = decoded[i]
            if self.test_cfg.get('tta', None) is not None:
                boxes = self.inverse_aug(new, boxes, img_metas[i])
            new.update_from_prediction(boxes, scores, labels, valid, to_ego=True)
            out_tracklets.append(new)
        out = dict(out_tracklets=out_tracklets)
        if self.test_cfg.get('test_occ_iou', False):
            out.update(self.test_occ(rois, res['fused_roi_feats'], gt_rois, gt_occ_list, gt_occ_score_list, pts_xyz,
                                     pts_batch_idx, pts_frame_inds, roi_frame_inds))
        if self.test_cfg.get('save_occ', False):
            # (the reference defines save_occ_from_tracklet and never calls it; test_cfg.save_occ is this package's key)
            check_save_occ_cfg(self.test_cfg)   # (again: the config may have changed since the head was built)
            self.save_occ_from_tracklet(tracklet_list, res)
        if self.test_cfg.get('save_gt_occ', False) and gt_rois is not None:
            check_save_gt_occ_cfg(self.test_cfg)
            self.save_gt_occ_from_tracklet(tracklet_list, res, gt_rois, gt_occ_list)
        return [out]

    # ------------------------------------------------------------------ online inference
    def online_begin(self, slots, device, cap=256, ring=False, long=False):
        """State for frame-by-frame inference over ``slots`` tracklets at a time (simple_test_step): the TemporalCache of
        the head's temporal transformer -- 2 * layers * cap * E * 4 bytes per slot, 9.4 MB for the ococcnet model at the
        default cap = 256 -- whose per-slot frame counter is also the frame index the next step of the slot gets.
        ``state.reset(slots)`` hands slots to new tracklets.  Tracklets of more than 256 frames: ``ring=True`` with
        cap >= test_cfg.attn_window_size > 0 (a windowed model: any length, 0.6 MB per slot at cap = 16), or ``long=True``
        with cap up to 4096 (a model that attends to all history)."""
        enc = self.bbox_head.trans_enc
        return OnlineState(TemporalCache(enc.num_layers, slots, self.bbox_head.roi_feature_channels, device, cap=cap,
                                         ring=ring, long=long))

    @torch.no_grad()
    def simple_test_step(self, pts_xyz, pts_feats, pts_batch_idx, boxes, scores, labels, slot, state, gt_rois=None,
                         occ=False, occ_transforms=None, tune=None):
        """One new frame of n tracklets: the frame's points (pts_batch_idx: the ROW 0..n-1 a point belongs to), the
        proposal boxes [n, 7], scores [n] and labels [n] of this frame, ``slot`` the list of the rows' slots in ``state``
        (online_begin).  Pools the frame's points into the frame's boxes, appends the RoI score / corner offsets as
        _bbox_forward does, runs OccBBoxHead.forward_step (the temporal transformer reads the slots' cached frames) and
        decodes with get_bboxes_from_tracklet.  The frame index of a row is the number of steps its slot has taken, which is
        what tracklets2rois gives offline.  Returns dict(boxes [n, 7], scores [n], labels [n], valid [n] -- RoIs without
        points are flagged, the caller keeps their proposal --, fused_roi_feats [n, D], ori_roi_feats [n, D]).

        ``occ=True`` adds the completed occupancy of the frame (``_step_occ``; csrc/occ_frame.hip): ``occ`` [N, 4] f32, the
        centres of the cells that the fused latent decodes as occupied or that one of the frame's points fell into, in the
        frame the inputs came in (through ``occ_transforms`` [n, 12] f32, a row-major 3x4 matrix per row, when given), and
        the cell's probability; ``occ_flags`` [N] uint8, bit 0 predicted and bit 1 observed; ``occ_counts``, the rows per
        input row as a list of int on the host.  Rows in input order, cells in grid order; the grid is that of the row's
        INPUT box, which the latent is relative to (as save_occ_from_tracklet takes the proposal RoIs).
        test_cfg.filter_empty_roi empties the rows whose box held no point; test_cfg.online_occ = dict(observed=True,
        chunk=1 << 20) turns the observed cells off or sets the decode's chunk.  Without ``occ`` nothing of this is launched.

        ``tune = dict(num_iter, downsample_size=-1, balance_sample=True, seed=0)`` (default: test_cfg.online_step_tuning, a
        key of this package, absent by default) tunes the fused shape latent of every row against the row's own points
        before score, box and occupancy are taken from it (OccBBoxHead.forward_step): ``fused_roi_feats`` is the
        tuned latent and ``occ`` is decoded from it; the temporal cache and ``ori_roi_feats`` are those of an untuned step.

        ALL frames of a tracklet must be given in ONE fixed coordinate frame: the encoders see absolute coordinates, so the
        cached keys and values belong to the frame they were computed in.  (The offline pipeline moves a tracklet into the
        ego pose of its middle frame, which an online caller cannot know; the first frame's pose serves.)

        Reported on the host before anything is launched: a step past the cache's cap and duplicate or out-of-range
        slots (OcoccError), CPU tensors (OcoccError), training mode (RuntimeError)."""
        if self.training:
            raise RuntimeError('simple_test_step is inference only: call .eval() first')
        return self._simple_test_rows(self.bbox_head.forward_step, state.cache.check_step(slot), None, pts_xyz, pts_feats,
                                      pts_batch_idx, boxes, scores, labels, state, gt_rois, occ, occ_transforms, tune)

    @torch.no_grad()
    def simple_test_steps(self, pts_xyz, pts_feats, pts_row_idx, boxes, scores, labels, slot_rows, state, gt_rois=None,
                          occ=False, tune=None, occ_transforms=None):
        """``simple_test_step`` for one OR MORE new frames per tracklet in one call -- a tracklet that arrives with
        history (a track confirmed after several hits, a dropped batch), or a recorded one fed T frames at a time.  A row
        is one (tracklet, frame): ``pts_row_idx`` the ROW 0..n-1 a point belongs to, boxes [n, 7], scores [n], labels [n]
        of the rows, ``slot_rows`` the slot of every row in ``state``.  The rows of a slot are its new frames, consecutive
        and in frame order ([3, 3, 3, 0, 5, 5]: three frames for slot 3, one for slot 0, two for slot 5); a slot's frames
        continue where its earlier steps stopped.  Pooling, decode and the returned dict are those of simple_test_step,
        n rows in input order; the temporal transformer takes all rows in one launch per layer
        (OccBBoxHead.forward_steps).  The coordinate-frame rule of simple_test_step holds, and ``occ=True`` adds its three
        keys ``occ``, ``occ_flags`` and ``occ_counts`` for the n rows (``occ_transforms`` [n, 12], per row, as there;
        default None); ``tune`` is that of simple_test_step, and a row draws the sample the single step of its (slot, frame)
        draws.

        Reported on the host before anything is launched: slots out of range, rows of a slot that are not consecutive, a
        run past the cache's cap (OcoccError), CPU tensors (OcoccError), training mode (RuntimeError)."""
        if self.training:
            raise RuntimeError('simple_test_steps is inference only: call .eval() first')
        slots, offsets, _ = state.cache.check_steps(slot_rows)
        return self._simple_test_rows(self.bbox_head.forward_steps, slots, offsets, pts_xyz, pts_feats, pts_row_idx, boxes,
                                      scores, labels, state, gt_rois, occ, occ_transforms, tune)

    def _simple_test_rows(self, head_step, slots, offsets, pts_xyz, pts_feats, pts_row_idx, boxes, scores, labels, state,
                          gt_rois, occ, occ_transforms, tune):
        """the body of simple_test_step (``offsets`` None: ``head_step`` is forward_step, which takes the rows' frame
        indices from here) and simple_test_steps (forward_steps, which derives them) over checked ``slots``: pool the
        rows' points into the rows' boxes, the head, the decode as one group, the result dict"""
        from . import _lib as L
        from .tracklet import host_index
        L.require_device(pts_xyz, pts_feats, pts_row_idx, boxes, scores, labels, state.cache.pos)
        n, dev = boxes.size(0), boxes.device
        if len(slots) != n or scores.size(0) != n or labels.size(0) != n:
            raise L.OcoccError(f'{len(slots)} slots, {scores.size(0)} scores, {labels.size(0)} labels for {n} boxes')
        if pts_xyz.size(0) == 0:   # (rows without points: one zero row, as the detector gives an empty sample)
            pts_xyz, pts_feats, pts_row_idx = TrackletDetectorOCC.fake_points_for_empty_input(
                [pts_xyz, pts_feats, pts_row_idx])
        rois = bbox3d2roi([boxes[i:i + 1, :7] for i in range(n)])     # column 0: the row's own index
        frames = (host_index([state.cache.pos_host[s] for s in slots], dev),) if offsets is None else ()
        same = torch.zeros((n,), dtype=torch.long, device=dev)          # (a row's points are its frame's: one frame key)
        pooled = self._pool_points(pts_xyz, pts_feats, pts_row_idx.long(), torch.zeros_like(pts_row_idx, dtype=torch.long),
                                   rois, scores, same)
        occ_cfg = self.online_occ_cfg() if occ else None               # (a wrong test_cfg.online_occ: before any launch)
        res = head_step(*pooled, rois, *frames, slots, state.cache, **self._step_kwargs(occ, tune))
        one = torch.cat([torch.zeros_like(rois[:, :1]), rois[:, 1:]], 1)   # (one group: get_bboxes splits by column 0)
        out_boxes, out_scores, out_labels, valid = self.bbox_head.get_bboxes_from_tracklet(
            one, res['cls_score'], res['bbox_pred'], res['nonempty_roi_mask'], labels, scores, None, gt_rois=gt_rois,
            cfg=self.test_cfg)[0]
        out = dict(boxes=out_boxes, scores=out_scores, labels=out_labels, valid=valid,
                   fused_roi_feats=res['fused_roi_feats'], ori_roi_feats=res['ori_roi_feats'])
        if occ:
            out.update(self._step_occ(res, rois, occ_cfg, occ_transforms))
        return out

    def _step_kwargs(self, occ, tune):
        """What a step adds to the head's call: the pooled points back for ``occ``, and the tuning of the latent -- the
        ``tune`` argument, or test_cfg.online_step_tuning when that is None.  Neither: nothing, the call of a plain step."""
        if tune is None:
            tune = self.test_cfg.get('online_step_tuning', None)
        kw = {'return_points': True} if occ else {}
        if tune is not None:
            kw['tune'] = tune
        return kw

    def online_occ_cfg(self):
        """test_cfg.online_occ: an optional dict, ``observed`` (default True: the cells the frame's points fell into join
        the predicted ones) and ``chunk`` (cells per decoder call, default 1 << 20 as get_occ_packed)"""
        cfg = self.test_cfg.get('online_occ', None) or {}
        if not isinstance(cfg, dict) or set(cfg) - {'observed', 'chunk'}:
            raise ValueError(f'test_cfg.online_occ is a dict with the keys observed and chunk, not {cfg!r}')
        chunk = cfg.get('chunk', 1 << 20)
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f'test_cfg.online_occ.chunk is the number of cells per decoder call, an int >= 1, not {chunk!r}')
        return dict(observed=bool(cfg.get('observed', True)), chunk=chunk)

    def online_merged_cfg(self, merged=True):
        """What ``merged`` of simple_test_scene_step asks for: test_cfg.online_merged (a key of this package, absent by
        default), overridden key by key by ``merged`` when that is a dict.  Keys: ``use_dim`` (the cloud's columns that are
        kept, default 5; an int n means range(n) as the reference's points_use_dim; 3 to 16 columns, x, y, z first),
        ``score_threshold`` (default 0.0: a cell survives iff its row's score is greater) and ``drop_observed`` (default
        False; True: a cell a real point of the frame fell into is left out).  Returns dict(use_dim as a tuple,
        score_threshold, drop_observed)."""
        from .occ.occ_ops import merge_use_dim
        keys = {'use_dim', 'score_threshold', 'drop_observed'}
        cfg = self.test_cfg.get('online_merged', None) or {}
        if not isinstance(cfg, dict) or set(cfg) - keys:
            raise ValueError(f'test_cfg.online_merged is a dict with the keys use_dim, score_threshold and drop_observed, not {cfg!r}')
        if isinstance(merged, dict):
            if set(merged) - keys:
                raise ValueError(f'merged is True or a dict with the keys use_dim, score_threshold and drop_observed, not {merged!r}')
            cfg = dict(cfg, **merged)
        elif merged is not True:
            raise ValueError(f'merged is True or a dict with the keys use_dim, score_threshold and drop_observed, not {merged!r}')
        use_dim, thr, drop = cfg.get('use_dim', 5), cfg.get('score_threshold', 0.0), cfg.get('drop_observed', False)
        try:
            dim = merge_use_dim(use_dim)
        except (TypeError, ValueError):
            dim = ()
        if not 3 <= len(dim) <= 16 or min(dim) < 0:
            raise ValueError(f'online_merged.use_dim is an int or a list of 3 to 16 column indices (x, y, z first), not {use_dim!r}')
        if isinstance(thr, bool) or not isinstance(thr, (int, float)):
            raise ValueError(f'online_merged.score_threshold is a number, not {thr!r}')
        if not isinstance(drop, bool):
            raise ValueError(f'online_merged.drop_observed is a bool, not {drop!r}')
        return dict(use_dim=dim, score_threshold=float(thr), drop_observed=drop)

    def _step_occ(self, res, rois, cfg, transforms=None):
        """The three ``occ`` keys of a step from what the head returned with return_points: the grid of every row's INPUT
        box decoded from the fused latent, joined with the cells the row's pooled points fell into
        (OccBBoxHead.get_frame_occ); test_cfg.filter_empty_roi goes down as the kernels' row_keep bytes."""
        keep = res['nonempty_roi_mask'] if self.test_cfg.get('filter_empty_roi', False) else None
        out, flags, counts = self.bbox_head.get_frame_occ(res['fused_roi_feats'], rois, res['local_xyz'], res['roi_inds'],
                                                          row_keep=keep, transforms=transforms, observed=cfg['observed'],
                                                          chunk=cfg['chunk'])
        return dict(occ=out, occ_flags=flags, occ_counts=counts)

    # PointsRangeFilter's range in the ococcnet pipelines (ococcnet_cfg.py) and LoadTrackletPoints' max_points there
    SCENE_ROWS_DEFAULTS = dict(extra_width=1.0, max_points=1024, attr_dims=2,
                               point_cloud_range=(-204.7, -204.7, -3.99, 204.7, 204.7, 7.99))

    @staticmethod
    def _boxes_through(boxes, m12):
        """boxes [n, 7] through the per-row 3x4 matrices m12 [n, 12] (float64, on the boxes' device) with the arithmetic
        of Tracklet.frame_transform: the centre through the matrix, the yaw by atan2 of the transformed heading vector
        (sin, cos, 0), the sizes kept; batched over the rows as Tracklet.shared2ego, in float64, rounded once."""
        m = m12.view(-1, 3, 4)
        b = boxes[:, :7].double()
        centre = (m[:, :, :3] * b[:, None, :3]).sum(-1) + m[:, :, 3]
        hv = torch.stack([torch.sin(b[:, 6]), torch.cos(b[:, 6])], 1)
        t = (m[:, :2, :2] * hv[:, None, :]).sum(-1)
        return torch.cat([centre, b[:, 3:6], torch.atan2(t[:, 0], t[:, 1])[:, None]], 1).to(boxes.dtype)

    @torch.no_grad()
    def simple_test_scene_step(self, points, pose, boxes, scores, labels, slot, state, gt_rois=None, occ=False, tune=None,
                               merged=None):
        """simple_test_step from what a sensor frame brings: ``points`` [N, >= 3 + attr] f32, the scene cloud of the frame in
        its own ego frame; ``pose``, the 4x4 ego -> world of the frame (numpy or torch); ``boxes`` [n, 7], ``scores`` [n],
        ``labels`` [n], the tracker's output for the frame in the same ego frame; ``slot`` and ``state`` as in
        simple_test_step.  Nothing has to be cropped, transformed, decorated or filtered beforehand.

        The fixed frame simple_test_step asks for is, per slot, the ego frame of the slot's FIRST step: the state keeps
        ``origin[slot]`` = inverse(pose) of that step (set when the slot's frame counter is 0, cleared by
        ``state.reset``).  Row i gets M_i = float32(origin[slot_i] @ pose); all pose arithmetic is float64 on the host and
        the matrices of a call go up in one copy.  scene_rows.scene_step_rows crops the cloud into the enlarged boxes, moves
        the points through M_i, decorates, filters and caps them (test_cfg.scene_rows: extra_width 1.0, max_points 1024,
        attr_dims 2, point_cloud_range that of the config's PointsRangeFilter); the boxes go through M_i as
        Tracklet.frame_transform moves them; then simple_test_step runs on the rows, unchanged.  ``gt_rois``, if given, is
        in the slots' fixed frames.

        Returns the dict of simple_test_step (boxes in the slots' fixed frames) and two more keys: ``boxes_ego`` [n, 7], the
        refined boxes back in the frame's ego frame through inverse(M_i), rows with valid == False their input box bit for
        bit; ``num_points`` [n] i64 on the host, the points in each enlarged box before the cap.  ``occ=True`` adds
        ``occ_ego`` [N, 4], the rows of simple_test_step's ``occ`` in the frame's ego frame -- through float32(inverse(M_i)),
        the matrix ``boxes_ego`` uses, applied in the fill kernel --, ``occ_flags`` and ``occ_counts``.  ``tune`` is that of
        simple_test_step.

        ``merged=True`` (test_cfg.online_merged, or a dict that overrides it: online_merged_cfg) implies ``occ=True`` and
        adds the occupancy-enhanced cloud of the frame, the array LoadPointsAndOccPredFromFile builds from files
        (occ_ops.occ_merge, csrc/occ_merge.hip): ``points_merged`` [N + K, D + 2] f32 -- ``points[:, use_dim]`` with two zero
        columns, then the surviving rows of ``occ_ego`` as x, y, z, D - 3 zeros, the row's score, 1 -- and
        ``merged_counts``, the survivors per input row as a list of int on the host.  The score of a row is what
        tools/online_raw.py writes into column 3 of its files: where(valid, refined score, input score) as f32.  Without
        ``merged`` nothing of this is launched and the keys are absent.  A frame without boxes (n == 0) with ``merged`` is
        not stepped: every key of the step is empty and ``points_merged`` is the cloud with its two zero columns.  Without
        ``merged`` n == 0 returns empty tensors for every key, launches nothing and leaves the state as it is; a slot's
        origin is stored once the rows are built, so a refused step leaves none behind (the chunked call's rules).

        Reported on the host before anything is launched: what simple_test_step reports, a pose that is not 4x4 or not
        finite (OcoccError), a slot in mid-tracklet without an origin -- it was stepped through simple_test_step
        (OcoccError), a wrong ``merged`` or test_cfg.online_merged (ValueError), a ``use_dim`` beyond the cloud's columns
        (OcoccError)."""
        import numpy as np
        from . import _lib as L
        if self.training:
            raise RuntimeError('simple_test_scene_step is inference only: call .eval() first')
        merged_cfg = None
        if merged is not None and merged is not False:
            merged_cfg, occ = self._merged_cfg_for(points, merged), True
        pose64 = np.asarray(pose.detach().cpu().numpy() if torch.is_tensor(pose) else pose, dtype=np.float64)
        if pose64.shape != (4, 4) or not np.isfinite(pose64).all():
            raise L.OcoccError(f'pose must be a finite 4x4 ego -> world matrix, got shape {pose64.shape}')
        return self._simple_test_scene_rows(points, None, pose64[None], boxes, scores, labels, slot, state, gt_rois, occ,
                                            tune, merged_cfg)

    def _merged_cfg_for(self, points, merged):
        """online_merged_cfg(merged), and its use_dim against the cloud's columns: what the merged forms check first"""
        from . import _lib as L
        cfg = self.online_merged_cfg(merged)
        if points.dim() != 2 or max(cfg['use_dim']) >= points.size(1):
            raise L.OcoccError(f'merged: use_dim {cfg["use_dim"]} of a cloud {tuple(points.shape)}')
        return cfg

    @staticmethod
    def _scene_frames(poses, cloud_sizes, frame_rows):
        """the frames arguments of a chunked scene call on the host: (poses as float64 [F, 4, 4] -- finite, one per
        cloud, or OcoccError --, (cloud_sizes, frame_rows) as lists of int)"""
        import numpy as np
        from . import _lib as L
        pose64 = np.asarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float64)
        sizes, frame_rows = [int(v) for v in cloud_sizes], [int(v) for v in frame_rows]
        F = len(sizes)
        if F == 0 and pose64.size == 0:
            pose64 = pose64.reshape(0, 4, 4)
        if pose64.shape != (F, 4, 4) or not np.isfinite(pose64).all():
            raise L.OcoccError(f'poses must be finite ego -> world matrices [F = {F}, 4, 4], one per cloud, got shape {pose64.shape}')
        return pose64, (sizes, frame_rows)

    def _simple_test_scene_rows(self, points, frames, pose64, boxes, scores, labels, slot, state, gt_rois, occ, tune,
                                merged_cfg):
        """the body of simple_test_scene_step (``frames`` None: one cloud under pose64 [1, 4, 4], every row its slot's
        first row, the one-cloud operators and simple_test_step) and of simple_test_scene_steps(_merged) (``frames`` =
        (cloud_sizes, frame_rows) as lists of int, pose64 [F, 4, 4]: the frames operators and simple_test_steps): the host
        checks in one order, the origins, the matrices in one copy, the rows, the step, the ego-frame keys, and with
        ``merged_cfg`` the merged cloud(s).  Nothing is launched and the state is untouched until every host check has
        passed; the origins are stored once the rows are built."""
        import numpy as np
        from . import _lib as L
        from .occ.occ_ops import occ_merge, occ_merge_frames
        from .scene_rows import scene_step_rows, scene_steps_rows
        from .tracklet import host_index
        F = len(pose64)
        if frames is None:
            slots = state.cache.check_step(slot)
            offsets = frame_rows = [0] * len(slots)
        else:
            sizes, frame_rows = frames
            slots, offsets, _ = state.cache.check_steps(slot)
        n = len(slots)
        if len(frame_rows) != n or any(not 0 <= f < F for f in frame_rows):
            raise L.OcoccError(f'frame_rows must hold the cloud 0..{F - 1} of each of the {n} rows, got {len(frame_rows)} values'
                               + (f' from {min(frame_rows)} to {max(frame_rows)}' if frame_rows else ''))
        for i in range(1, n):
            if offsets[i] and frame_rows[i] <= frame_rows[i - 1]:
                raise L.OcoccError(f'the rows of slot {slots[i]} go from cloud {frame_rows[i - 1]} to cloud {frame_rows[i]}: '
                                   'within a slot\'s run frame_rows is strictly increasing (its frames in time order, none twice)')
        inverse, started, origins = {}, {}, []
        for i, s in enumerate(slots):
            if offsets[i] == 0 and state.frames[s] == 0:                # a slot that starts here: its first row's cloud
                f = frame_rows[i]
                if f not in inverse:
                    try:
                        inverse[f] = np.linalg.inv(pose64[f])
                    except np.linalg.LinAlgError:
                        raise L.OcoccError(f'pose {f} is singular: not an ego -> world transform')
                started[s] = inverse[f]
            if s in started:
                origins.append(started[s])
            elif state.origin[s] is None:
                raise L.OcoccError(f'slot {s} holds {state.frames[s]} frames and no origin: it was stepped through '
                                   'simple_test_step, whose caller keeps the fixed frame (reset the slot)')
            else:
                origins.append(state.origin[s])
        if boxes.size(0) != n or scores.size(0) != n or labels.size(0) != n:
            raise L.OcoccError(f'{n} slots, {scores.size(0)} scores, {labels.size(0)} labels for {boxes.size(0)} boxes')
        if frames is not None and (points.dim() != 2 or sum(sizes) != points.size(0) or min(sizes, default=0) < 0):
            raise L.OcoccError(f'cloud_sizes must be >= 0 and sum to the points given, got {sum(sizes)} for {tuple(points.shape)}')
        L.require_device(points, boxes, scores, labels, state.cache.pos)
        dev = boxes.device
        if n == 0:                                                      # nothing to step: every key empty, no launch
            feats = boxes.new_zeros((0, self.bbox_head.roi_feature_channels))
            out = dict(boxes=boxes.new_zeros((0, 7)), scores=scores.new_zeros((0,)), labels=labels.new_zeros((0,)),
                       valid=torch.zeros((0,), dtype=torch.bool, device=dev), fused_roi_feats=feats, ori_roi_feats=feats,
                       boxes_ego=boxes.new_zeros((0, 7)), num_points=torch.zeros((0,), dtype=torch.long))
            if occ:
                out.update(occ_ego=boxes.new_zeros((0, 4)), occ_flags=torch.zeros((0,), dtype=torch.uint8, device=dev),
                           occ_counts=[])
        else:
            cfg = dict(self.SCENE_ROWS_DEFAULTS, **(self.test_cfg.get('scene_rows', None) or {}))
            if occ:
                self.online_occ_cfg()                                   # (a wrong test_cfg.online_occ: before the origins)
            to_fixed = np.stack([o @ pose64[f] for o, f in zip(origins, frame_rows)])
            try:
                from_fixed = np.linalg.inv(to_fixed)
            except np.linalg.LinAlgError:
                raise L.OcoccError('a pose is singular: not an ego -> world transform')
            mats = host_index(np.stack([to_fixed[:, :3].reshape(n, 12), from_fixed[:, :3].reshape(n, 12)]), dev,
                              dtype=torch.float64)                     # [2, n, 12]: M and inverse(M), one copy
            fixed_boxes = self._boxes_through(boxes, mats[0])
            rows_kw = dict(transforms=mats[0].float(), extra_width=cfg['extra_width'], attr_dims=cfg['attr_dims'],
                           point_cloud_range=cfg['point_cloud_range'], max_points=cfg['max_points'], deco_boxes=fixed_boxes)
            if frames is None:
                step, rows = self.simple_test_step, scene_step_rows(points, boxes, scores, **rows_kw)
            else:
                step, rows = self.simple_test_steps, scene_steps_rows(points, sizes, boxes, scores, frame_rows, **rows_kw)
            for s, o in started.items():                                # (every host check has passed)
                state.origin[s] = o
            kw = dict(occ=True, occ_transforms=mats[1].float()) if occ else {}
            out = step(*rows[:3], fixed_boxes, scores, labels, slots, state, gt_rois=gt_rois, tune=tune, **kw)
            if occ:
                out['occ_ego'] = out.pop('occ')
            out['boxes_ego'] = torch.where(out['valid'].to(dev).bool()[:, None], self._boxes_through(out['boxes'], mats[1]),
                                           boxes[:, :7])
            out['num_points'] = rows[3]
        if merged_cfg is not None:
            row_score = torch.where(out['valid'].to(dev).bool(), out['scores'].float(), scores.float())
            kw = dict(row_score=row_score, flags=out['occ_flags'], drop_observed=merged_cfg['drop_observed'],
                      score_threshold=merged_cfg['score_threshold'])
            if frames is None:
                out['points_merged'], out['merged_counts'] = occ_merge(
                    points, out['occ_ego'], out['occ_counts'], merged_cfg['use_dim'], **kw)
            else:
                out['points_merged'], out['merged_offsets'], out['merged_counts'] = occ_merge_frames(
                    points, sizes, out['occ_ego'], out['occ_counts'], frame_rows, merged_cfg['use_dim'], **kw)
        return out

    @torch.no_grad()
    def simple_test_scene_steps(self, points, cloud_sizes, poses, boxes, scores, labels, frame_rows, slot_rows, state,
                                gt_rois=None, occ=False, tune=None):
        """simple_test_steps from what SEVERAL sensor frames bring -- a track confirmed after three hits comes with three
        boxes in three clouds under three poses: ``points`` [N, >= 3 + attr] f32, the F scene clouds concatenated, each in its
        own ego frame, ``cloud_sizes`` their F lengths (ints on the host), ``poses`` [F, 4, 4] the ego -> world pose of each
        cloud (numpy or torch).  A row is one (tracklet, frame) exactly as in simple_test_steps: ``boxes`` [n, 7] each in the
        ego frame of the row's own cloud, ``scores`` [n], ``labels`` [n], ``frame_rows`` the cloud 0..F-1 of every row,
        ``slot_rows`` its slot; the rows of a slot are consecutive and in frame order, so within a slot's run ``frame_rows``
        is strictly increasing (gaps are fine: a track may miss a frame).

        Origins as in simple_test_scene_step: a slot whose frame counter is 0 takes inverse(pose of its FIRST row's cloud),
        any other slot ``state.origin[slot]``; they are stored only after every host check has passed.  Row i gets
        M_i = float32(origin[slot_i] @ poses[frame_rows[i]]) (float64 on the host; M and inverse(M) of all rows go up in
        one copy), the boxes go through M_i, scene_rows.scene_steps_rows builds the rows of ALL clouds with one count launch,
        one read-back and one fill launch (test_cfg.scene_rows as in the single step), and simple_test_steps runs on them.

        Returns the keys of simple_test_scene_step for the n rows in input order: the dict of simple_test_steps,
        ``boxes_ego`` (rows with valid == False their input box bit for bit), ``num_points`` [n] i64 on the host (uncapped),
        and with ``occ=True`` ``occ_ego`` (each row's cells in the ego frame of ITS cloud), ``occ_flags``, ``occ_counts``.
        ``tune`` passes through.  n == 0 returns empty tensors for every key, launches nothing and leaves the state as it is.

        The occupancy-enhanced clouds of the F frames of such a call come from simple_test_scene_steps_merged, which runs
        this call with ``occ=True`` and merges all F clouds with one count launch, one read-back and one fill launch.

        Reported on the host before anything is launched: what simple_test_steps reports, poses that are not [F, 4, 4], not
        finite or singular, cloud_sizes of another length than F, frame_rows outside 0..F-1, repeating or going back inside
        a slot's run, a slot in mid-tracklet without an origin (OcoccError), training mode (RuntimeError)."""
        if self.training:
            raise RuntimeError('simple_test_scene_steps is inference only: call .eval() first')
        pose64, frames = self._scene_frames(poses, cloud_sizes, frame_rows)
        return self._simple_test_scene_rows(points, frames, pose64, boxes, scores, labels, slot_rows, state, gt_rois, occ,
                                            tune, None)

    @torch.no_grad()
    def simple_test_scene_steps_merged(self, points, cloud_sizes, poses, boxes, scores, labels, frame_rows, slot_rows, state,
                                       merged=True, gt_rois=None, tune=None):
        """simple_test_scene_steps with ``occ=True`` and the occupancy-enhanced cloud of EVERY frame of the call, the arrays
        F calls of simple_test_scene_step(merged=...) return as ``points_merged``, in one array: ``merged`` is True
        (test_cfg.online_merged) or a dict that overrides it (online_merged_cfg); the other arguments are those of
        simple_test_scene_steps.

        Returns the dict of simple_test_scene_steps(..., occ=True) and three more keys: ``points_merged`` [N + K, D + 2]
        f32, frame after frame -- the rows of cloud f as ``points[:, use_dim]`` with two zero columns, then the surviving
        cells of the rows with frame_rows[i] == f in ascending i as x, y, z, D - 3 zeros, the row's score, 1 --,
        ``merged_offsets``, F + 1 ints on the host: frame f is points_merged[merged_offsets[f]:merged_offsets[f + 1]], and
        ``merged_counts``, the survivors per input row as a list of int on the host.  The score of a row is
        where(valid, refined score, input score) as f32, the rule of simple_test_scene_step.  All F clouds are merged by
        occ_ops.occ_merge_frames: one count launch, one read-back and one fill launch, whatever F.

        With n == 0 nothing is stepped and the state is as it was: ``points_merged`` is the F clouds with their two zero
        columns and ``merged_offsets`` the prefix of cloud_sizes.

        Reported on the host before anything is launched: what simple_test_scene_steps reports, a wrong ``merged`` or
        test_cfg.online_merged (ValueError), a ``use_dim`` beyond the cloud's columns (OcoccError)."""
        if self.training:
            raise RuntimeError('simple_test_scene_steps_merged is inference only: call .eval() first')
        merged_cfg = self._merged_cfg_for(points, merged)
        pose64, frames = self._scene_frames(poses, cloud_sizes, frame_rows)
        return self._simple_test_scene_rows(points, frames, pose64, boxes, scores, labels, slot_rows, state, gt_rois, True,
                                            tune, merged_cfg)

    def online_chunk(self):
        """test_cfg.online_chunk: the frames simple_test_online feeds per call, an int >= 1 (default 1: single steps)"""
        chunk = self.test_cfg.get('online_chunk', 1)
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f'test_cfg.online_chunk is the number of frames per call, an int >= 1, not {chunk!r}')
        return chunk

    @torch.no_grad()
    def simple_test_online(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, img_metas, tracklet_list,
                           gt_candidates_list=None, gt_occs_list=None, gt_occ_scores_list=None, **kwargs):
        """simple_test computed the way the method is deployed: the tracklet is fed to simple_test_step frame by frame in
        one slot of a fresh state, then test_occ / the exports run on the concatenated per-step features.  Same arguments,
        same result (the temporal transformer is causal: frame t never saw the later frames offline either); what
        simple_test does when test_cfg.online is set.  The points are taken in the coordinate frame they come in.
        test_cfg.online_chunk = T > 1: T frames per simple_test_steps call instead (the last call takes the rest), through
        the same cache -- a ring of W rows takes chunks longer than W.
        Up to 256 frames: a cache of that many rows.  Above: with test_cfg.attn_window_size = W > 0 a ring cache of W rows
        (any length), without a window a long cache of up to 4096 rows; past that an OcoccError."""
        from . import _lib as L
        assert len(tracklet_list) == 1, 'only support batch size 1'
        if self.test_cfg.get('tta', None) is not None:
            raise NotImplementedError('test_cfg.online with test_cfg.tta')
        chunk = self.online_chunk()
        num = len(tracklet_list[0])
        window = self.test_cfg.get('attn_window_size', -1)
        if num <= 256:
            cache_kw = dict(cap=max(num, 1))
        elif window > 0:       # (only ever reads the last ``window`` frames: a ring of that many rows, any length)
            cache_kw = dict(cap=window, ring=True)
        elif num <= TemporalCache.MAX_LONG_CAP:
            cache_kw = dict(cap=num, long=True)
        else:
            raise L.OcoccError(f'a tracklet of {num} frames without test_cfg.attn_window_size: the K/V cache of online '
                               f'inference holds at most {TemporalCache.MAX_LONG_CAP} frames of history')
        L.require_device(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds)
        gt_rois, gt_occ_list, gt_occ_score_list = self._test_gt_rois(tracklet_list, gt_candidates_list, gt_occs_list,
                                                                     gt_occ_scores_list)
        rois, roi_frame_inds, cls_preds, labels_3d = self.tracklets2rois(tracklet_list)
        state = self.online_begin(1, rois.device, **cache_kw)
        # the points frame by frame: one stable sort, the counts in one read-back
        order = torch.sort(pts_frame_inds, stable=True).indices
        counts = torch.bincount(pts_frame_inds, minlength=num).tolist()
        assert len(counts) == num, 'a point lies in a frame past the tracklet'
        steps, first = [], 0
        for t in range(0, num, chunk):   # T frames per call, the last call takes the rest
            T = min(chunk, num - t)
            sel = order[first:first + sum(counts[t:t + T])]
            first += sel.numel()
            rows = (rois[t:t + T, 1:8], cls_preds[t:t + T], labels_3d[t:t + T])
            gt = None if gt_rois is None else gt_rois[t:t + T]
            if chunk == 1:
                steps.append(self.simple_test_step(pts_xyz[sel], pts_feats[sel], torch.zeros_like(pts_batch_idx[sel]), *rows,
                                                   [0], state, gt_rois=gt))
            else:   # (a point's row is its frame's place in the chunk)
                steps.append(self.simple_test_steps(pts_xyz[sel], pts_feats[sel], pts_frame_inds[sel] - t, *rows, [0] * T,
                                                    state, gt_rois=gt))
        cat = lambda k: torch.cat([s[k] for s in steps], 0)
        res = dict(fused_roi_feats=cat('fused_roi_feats'), ori_roi_feats=cat('ori_roi_feats'), nonempty_roi_mask=cat('valid'))
        decoded = [(cat('boxes'), cat('scores'), cat('labels'), cat('valid'))]
        return self._test_results(tracklet_list, decoded, res, rois, roi_frame_inds, img_metas, gt_rois, gt_occ_list,
                                  gt_occ_score_list, pts_xyz, pts_batch_idx, pts_frame_inds)

    @torch.no_grad()
    def save_occ_from_tracklet(self, tracklet_list, bbox_results, gt_tracklet_list=None, gt_occ_list=None,
                               gt_occ_score_list=None, save_gt_occ=False, gt_score=None):
        """The completed occupancy of one tracklet as files (tracklet_roi_head_occ.py:612-745, prediction branch):
        ``<test_cfg.occ_save_root>/<segment>/<timestamp>/<type>_<id>.bin`` per frame, float32 [n, 4]: the occupied cell
        centres of get_occ(fused features, transform=True) and the frame's box score (``gt_score[i]`` when given) in
        every row.  Frames under test_cfg.min_evaluate_length are not written, nor (test_cfg.filter_empty_roi) frames
        whose RoI had no points.  One packed array per tracklet (bbox_head.get_occ_packed), one device-to-host copy,
        sliced on the host (occ_export.write_tracklet_occ).  Returns the paths written.  The ground-truth branch
        (save_gt_occ=True) is save_gt_occ_from_tracklet, a method of its own."""
        from . import occ_export
        assert len(tracklet_list) == 1, 'only support batch size 1'
        if save_gt_occ:
            raise NotImplementedError(
                'save_occ_from_tracklet(save_gt_occ=True): the reference\'s ground-truth branch crops the labels with '
                'points_in_boxes_gpu of the roiaware_pool3d extension, which is outside this package\'s scope; only the '
                'predicted occupancy is exported')
        tracklet = tracklet_list[0]
        rois, _, _, _ = self.tracklets2rois([tracklet])
        feats = bbox_results['fused_roi_feats']
        score_list = tracklet.concated_scores()
        if gt_score is not None:
            assert len(score_list) == len(gt_score), f'{len(score_list)} != {len(gt_score)}'
            score_list = torch.as_tensor(gt_score, dtype=torch.float32)
        scores = score_list.detach().to(device=feats.device, dtype=torch.float32)
        packed, counts = self.bbox_head.get_occ_packed(feats, rois, transform=True, roi_values=scores)
        skip = set(range(min(self.test_cfg.get('min_evaluate_length', 0), len(counts))))
        if self.test_cfg.get('filter_empty_roi', False):
            nonempty = bbox_results['nonempty_roi_mask'].tolist()
            for i in range(len(counts)):
                if i not in skip and not nonempty[i]:
                    print(f'empty roi {i} in {tracklet.segment_name} at {tracklet.ts_list[i]}')
                    skip.add(i)
        return occ_export.write_tracklet_occ(self.test_cfg['occ_save_root'], tracklet.segment_name, tracklet.ts_list,
                                             tracklet.type, tracklet.id, packed.cpu().numpy(), counts, skip)

    @torch.no_grad()
    def save_gt_occ_from_tracklet(self, tracklet_list, bbox_results, gt_rois, gt_occ_list, root=None):
        """The annotated occupancy of the matched GT track as files, cropped to the proposal boxes (the save_gt_occ=True
        branch of the reference's save_occ_from_tracklet, tracklet_roi_head_occ.py:634-702): for every frame of the
        proposal tracklet that has a GT box (``gt_rois[:, 0] == 1``; gt_rois as get_gt_rois returns it, aligned to the
        proposal's ts_list) the occupied label cells ``gt_occ[..., :3][gt_occ[..., 3] == 1]`` are moved into that
        frame's LiDAR frame by the GT box and those inside the proposal box are written to
        ``<test_cfg.gt_occ_save_root>/<segment>/<timestamp>/<type>_<id>.bin``, float32 [n, 4] with score 1, under the
        proposal's segment, type and id.  Nothing is written (``[]``) without labels, without a matched frame or without
        an occupied cell.  test_cfg.min_evaluate_length and filter_empty_roi apply to the frame's index in the PROPOSAL
        tracklet (the reference indexes its filtered list against the unfiltered mask: not reproduced).  One packed
        array per tracklet (bbox.crop_gt_occ_packed), one device-to-host copy.  Returns the paths written."""
        from . import occ_export
        from .bbox import crop_gt_occ_packed
        from .tracklet import host_index
        assert len(tracklet_list) == 1, 'only support batch size 1'
        tracklet = tracklet_list[0]
        if gt_rois is None or gt_occ_list is None or gt_occ_list[0] is None:
            return []
        assert gt_rois.size(0) == len(tracklet), f'{gt_rois.size(0)} gt_rois for {len(tracklet)} frames'
        frames = [i for i, m in enumerate((gt_rois[:, 0] == 1).tolist()) if m]
        if not frames:
            return []
        occ = gt_occ_list[0]
        cells = occ[..., :3][occ[..., 3] == 1].float()
        if cells.size(0) == 0:
            return []
        rois, _, _, _ = self.tracklets2rois([tracklet])
        dev = rois.device
        idx = host_index(frames, dev)
        packed, counts = crop_gt_occ_packed(cells.to(dev), gt_rois.to(dev)[idx][:, 1:8], rois[idx][:, 1:8])
        low = self.test_cfg.get('min_evaluate_length', 0)
        skip = {k for k, i in enumerate(frames) if i < low}
        if self.test_cfg.get('filter_empty_roi', False):
            nonempty = bbox_results['nonempty_roi_mask'].tolist()
            for k, i in enumerate(frames):
                if k not in skip and not nonempty[i]:
                    print(f'empty roi {i} in {tracklet.segment_name} at {tracklet.ts_list[i]}')
                    skip.add(k)
        root = root if root is not None else self.test_cfg['gt_occ_save_root']
        return occ_export.write_tracklet_occ(root, tracklet.segment_name, [tracklet.ts_list[i] for i in frames],
                                             tracklet.type, tracklet.id, packed.cpu().numpy(), counts, skip)

    @staticmethod
    def inverse_aug(trk, boxes, meta):
        """Undo the test-time augmentation recorded in the sample's meta on the refined boxes [L,7] and on the
        tracklet they refine (tracklet_roi_head_occ.py:746-757): flips first, then the rotation."""
        holder = Tracklet(boxes, list(range(boxes.size(0))))
        if meta.get('pcd_horizontal_flip', False):
            holder.flip('horizontal')
            trk.flip('horizontal')
        if meta.get('pcd_vertical_flip', False):
            holder.flip('vertical')
            trk.flip('vertical')
        if 'pcd_rot_angle' in meta:
            assert getattr(trk, 'rot_angle', meta['pcd_rot_angle']) == meta['pcd_rot_angle']
            holder.rotate(-meta['pcd_rot_angle'])
            trk.rotate(-meta['pcd_rot_angle'])
        return holder.boxes

    @torch.no_grad()
    def test_occ(self, rois, fused_roi_feats, gt_rois, gt_occ_list, gt_occ_score_list, pts_xyz=None,
                 pts_batch_idx=None, pts_frame_inds=None, roi_frame_inds=None):
        """Occupancy IoU counts of one tracklet (tracklet_roi_head_occ.py:268-486): every known GT voxel is
        decoded in every RoI that has a GT box at its timestamp, in chunks of test_cfg.iou_chunk_size RoIs;
        integer inter / union per RoI.  Nothing is counted without occupancy labels, without a matched frame,
        or when the label confidence is under occ_label_thresh.  The decoder is called with (features, points,
        RoI index) -- no [chunk,K,1536] copies.  test_cfg.test_baseline (:289-393) rasterises the points
        accumulated up to each frame instead of decoding."""
        empty = dict(inters=[], unions=[], gt_boxes=[])
        if gt_rois is None or gt_occ_list is None or gt_occ_list[0] is None:
            return empty
        match = gt_rois[:, 0] == 1
        if not bool(match.any()) or float(gt_occ_score_list[0]) < self.bbox_head.occ_label_thresh:
            return empty
        occ_xyz, occ_label = gt_occ_list[0][..., :3], (gt_occ_list[0][..., 3] == 1).long()
        K = occ_xyz.size(0)

        def to_roi_frame(xyz, gb, pb):
            if not self.test_cfg.get('transform_to_gt', True):
                return xyz
            return points_box_to_box(xyz, gb, pb)   # GT box frame -> ego frame -> RoI frame (labels sit at voxel gravity centres)

        if self.test_cfg.get('test_baseline', False):
            return self._test_occ_accumulated_points(rois, gt_rois, match, occ_xyz, occ_label, to_roi_frame, pts_xyz,
                                                     pts_batch_idx, pts_frame_inds, roi_frame_inds)
        chunk = self.test_cfg.get('iou_chunk_size', -1)
        chunk = int(match.numel()) if chunk == -1 else chunk
        pred_boxes, gt_boxes_all, feats = rois[match][:, 1:], gt_rois[match][:, 1:], fused_roi_feats[match]
        decoder = self.bbox_head.occ_ae_head.occ_decoder
        outside = self.test_cfg.get('ignore_outside_occ', False)
        if OCC_IOU_KERNEL and decoder.cls_dim == 1 and feats.is_cuda:
            # the counts stay on the device: one int64 [R, 2] buffer per tracklet, one count launch after each chunk's
            # decoder launch, ONE read-back at the end (csrc/occ_iou_count.hip)
            R = gt_boxes_all.size(0)
            counts = torch.zeros((R, 2), dtype=torch.long, device=feats.device)
            halves = (pred_boxes[:, 3:6] / 2).contiguous() if outside else None
            sizes, row0 = [], 0
            for f, pb, gb in zip(torch.split(feats, chunk), torch.split(pred_boxes, chunk),
                                 torch.split(gt_boxes_all, chunk)):
                n = gb.size(0)
                xyz = to_roi_frame(occ_xyz[None].repeat(n, 1, 1), gb, pb)
                idx = torch.arange(n, device=xyz.device).repeat_interleave(K)
                logits = decoder(f, xyz.reshape(n * K, 3), idx)
                occ_ops.occ_iou_count(logits, occ_label, counts, row0, decoder.pos_thresh,
                                      xyz if outside else None, halves[row0:row0 + n] if outside else None)
                sizes.append(n)
                row0 += n
            host = counts.cpu().t().contiguous()
            return dict(inters=[t.clone() for t in host[0].split(sizes)],
                        unions=[t.clone() for t in host[1].split(sizes)],
                        gt_boxes=[t.clone() for t in gt_boxes_all.cpu().split(sizes)])
        inters, unions, gt_boxes = [], [], []
        for f, pb, gb in zip(torch.split(feats, chunk), torch.split(pred_boxes, chunk), torch.split(gt_boxes_all, chunk)):
            n = gb.size(0)
            xyz = to_roi_frame(occ_xyz[None].repeat(n, 1, 1), gb, pb)
            idx = torch.arange(n, device=xyz.device).repeat_interleave(K)
            logits = decoder(f, xyz.reshape(n * K, 3), idx)
            inter, union = occ_iou_counts_aten(decoder, logits, occ_label, xyz, pb[:, 3:6] / 2 if outside else None)
            inters.append(inter.cpu())
            unions.append(union.cpu())
            gt_boxes.append(gb.cpu())
        return dict(inters=inters, unions=unions, gt_boxes=gt_boxes)

    def _test_occ_accumulated_points(self, rois, gt_rois, match, occ_xyz, occ_label, to_roi_frame, pts_xyz,
                                     pts_batch_idx, pts_frame_inds, roi_frame_inds):
        """The point-accumulation baseline (:289-393): the occupancy of RoI i is the set of 0.2 m cells of its own
        box hit by the pooled points of RoIs 0..i, each in its own RoI frame."""
        inds, roi_inds, info = self.roi_extractor(pts_xyz[:, :3], pts_batch_idx, pts_frame_inds, rois[:, :8],
                                                  roi_frame_inds)
        local = rotation_3d_in_axis(info['local_xyz'][None], info['local_xyz'].new_tensor([torch.pi / 2]), axis=2)[0]
        vs = self.bbox_head.occ_ae_head.voxel_size
        inters, unions, gt_boxes = [], [], []
        for i in torch.nonzero(match).view(-1).tolist():
            gb, pb = gt_rois[i, 1:], rois[i, 1:]
            q = to_roi_frame(occ_xyz[None].clone(), gb[None], pb[None])[0]
            size = pb[3:6]
            dims = torch.ceil(size / vs).to(torch.int32)
            cells = lambda p: torch.floor((p + size[None] / 2) / vs).to(torch.long)
            inb = lambda c: (c >= 0).all(1) & (c < dims[None]).all(1)
            pc = cells(local[roi_inds <= i])
            pc = pc[inb(pc)]
            qc = cells(q)
            qin = inb(qc)
            pred = torch.zeros_like(occ_label)
            if bool(qin.any()):
                grid = torch.zeros(tuple(int(d) for d in dims), dtype=torch.bool, device=q.device)
                grid[pc[:, 0], pc[:, 1], pc[:, 2]] = True
                pred[qin] = grid[qc[qin, 0], qc[qin, 1], qc[qin, 2]].long()
            inters.append(((pred == 1) & (occ_label == 1)).sum(-1, keepdim=True).cpu())
            unions.append(((pred == 1) | (occ_label == 1)).sum(-1, keepdim=True).cpu())
            gt_boxes.append(gb[None])
        return dict(inters=inters, unions=unions, gt_boxes=gt_boxes)


@DETECTORS.register_module()
class TrackletDetectorOCC(nn.Module):
    """Concatenate the per-sample point lists, build batch / frame indices, call the RoI head
    (tracklet_detector_occ.py:96-198).  Points: [n_i, 3 + C] with xyz first; the decorated
    features (intensity, elongation, yaw/pi, size/10 x3, score) follow."""

    def __init__(self, roi_head, train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None, **kwargs):
        super().__init__()
        rh = dict(roi_head)
        rh['train_cfg'], rh['test_cfg'] = train_cfg, test_cfg
        self.roi_head = HEADS.build(rh)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    @staticmethod
    def _cat_points(points, pts_frame_inds):
        xyz = torch.cat([p[:, :3] for p in points], 0)
        feats = torch.cat([p[:, 3:] for p in points], 0)
        # (sample index of every point: one repeat with the counts known on the host -- no fill per sample, no read-back)
        from .tracklet import host_index
        dev = points[0].device
        counts = [int(p.size(0)) for p in points]
        batch = torch.repeat_interleave(torch.arange(len(points), device=dev), host_index(counts, dev), output_size=sum(counts))
        return xyz.contiguous(), feats.contiguous(), batch, torch.cat(pts_frame_inds, 0).long()

    @staticmethod
    def fake_points_for_empty_input(tensors):
        """After PointsRangeFilter a sample can arrive without points: give it one zero row
        (tracklet_detector_occ.py:299-311)."""
        return [t.new_zeros((1,) + tuple(t.shape[1:])) if len(t) == 0 else t for t in tensors]

    def forward_train(self, points, pts_frame_inds=None, img_metas=None, tracklet=None, gt_tracklet_candidates=None,
                      occ_labels=None, occ_labels_scores=None):
        """tracklet_detector_occ.py:96-147 (argument names = the keys Collect3D emits, ococcnet.py:247-254)."""
        points = self.fake_points_for_empty_input(points)
        pts_frame_inds = self.fake_points_for_empty_input(pts_frame_inds)
        xyz, feats, batch, frames = self._cat_points(points, pts_frame_inds)
        return self.roi_head.forward_train(pts_xyz=xyz, pts_feats=feats, pts_batch_idx=batch, pts_frame_inds=frames,
                                           img_metas=img_metas, tracklet_list=tracklet,
                                           gt_candidates_list=gt_tracklet_candidates, gt_occs_list=occ_labels,
                                           gt_occ_scores_list=occ_labels_scores)

    def simple_test(self, points, img_metas, pts_frame_inds, tracklet, gt_tracklet_candidates=None, occ_labels=None,
                    occ_labels_scores=None, rescale=False, **kwargs):
        """tracklet_detector_occ.py:149-198."""
        points = self.fake_points_for_empty_input(points)
        pts_frame_inds = self.fake_points_for_empty_input(pts_frame_inds)
        xyz, feats, batch, frames = self._cat_points(points, pts_frame_inds)
        return self.roi_head.simple_test(pts_xyz=xyz, pts_feats=feats, pts_batch_idx=batch, pts_frame_inds=frames,
                                         img_metas=img_metas, tracklet_list=tracklet,
                                         gt_candidates_list=gt_tracklet_candidates, gt_occs_list=occ_labels,
                                         gt_occ_scores_list=occ_labels_scores)

    def forward_test(self, points, img_metas, img=None, **kwargs):
        """tracklet_detector_occ.py:313-345: with test_cfg.tta the arguments are lists over augmentations."""
        if self.test_cfg is not None and self.test_cfg.get('tta', None) is not None:
            return self.aug_test(points, img_metas, **kwargs)
        return self.simple_test(points, img_metas, **kwargs)

    def aug_test(self, points, img_metas, pts_frame_inds, tracklet, rescale=False):
        """Test-time augmentation (tracklet_detector_occ.py:200-221): points / metas / frame indices / tracklets
        are lists over the augmentations, each a batch of ONE sample; every augmentation is refined on its own,
        its boxes are mapped back through the augmentation (TrackletRoIHeadOCC.inverse_aug) and the per-frame
        boxes are merged with Tracklet.merge_augs under test_cfg['tta'].  Returns one merged Tracklet per sample."""
        assert len(points) == len(img_metas) == len(pts_frame_inds) == len(tracklet)
        if self.roi_head.test_cfg.get('online', False):
            raise NotImplementedError('test_cfg.online with test-time augmentation: every augmentation would need its own '
                                      'K/V cache; refine the augmented tracklets offline')
        tta = self.roi_head.test_cfg['tta']
        per_aug = []
        for p, meta, inds, trks in zip(points, img_metas, pts_frame_inds, tracklet):
            outs = []
            for i, trk in enumerate(trks):  # simple_test refines one tracklet per call and undoes the augmentation
                r = self.simple_test([p[i]], [meta[i]], [inds[i]], [trk])[0]
                outs.append(r['out_tracklets'][0])
            per_aug.append(outs)
        bsz = len(points[0])
        return [Tracklet.merge_augs([per_aug[k][i] for k in range(len(points))], tta, points[0][0].device)
                for i in range(bsz)]

    def forward(self, return_loss=True, **kwargs):
        return self.forward_train(**kwargs) if return_loss else self.forward_test(**kwargs)


def occ_iou_counts_aten(decoder, logits, occ_label, xyz, half=None):
    """The ATen form of one chunk's occupancy counts in test_occ (tracklet_roi_head_occ.py:459-486), kept for
    OCOCC_OCC_IOU_KERNEL=0, for cls_dim > 1 and as the yardstick of csrc/occ_iou_count.hip: logits [n*K, cls_dim] of
    the query points xyz [n, K, 3] (RoI frame), occ_label [K] long; with half [n, 3] (ignore_outside_occ) a cell outside
    -half <= xyz <= half is predicted empty.  -> inter [n], union [n] (int64, on the device)."""
    n, K = xyz.size(0), xyz.size(1)
    lab = occ_label[None].repeat(n, 1)
    if half is not None:
        half = half[:, None]
        inside = (xyz >= -half).all(-1) & (xyz <= half).all(-1)
    else:
        inside = torch.ones((n, K), dtype=torch.bool, device=xyz.device)
    cls = decoder.get_cls_from_pred(logits).view(n, K) * inside
    return ((cls == 1) & (lab == 1)).sum(1), ((cls == 1) | (lab == 1)).sum(1)


def occupancy_iou_metrics(results):
    """Aggregate per-RoI (inter, union, gt box) lists exactly as WaymoTrackletDatasetWithOcc.evaluate
    does for metric 'iou' (mmdet3d/datasets/waymo_tracklet_dataset.py:629-672): overall IoU =
    sum inter / sum union, mIoU over tracklets, mIoU over boxes, and the mean box IoU by GT
    volume (<30, [30,150), >=150 m^3)."""
    total_inter = total_union = 0.0
    track, box, small, medium, large = [], [], [], [], []
    for r in results:
        if 'inters' not in r or (len(r['inters']) == 0 and len(r['unions']) == 0):
            continue
        inters = torch.cat(r['inters'], 0)
        unions = torch.cat(r['unions'], 0)
        box_ious = inters / unions
        box.extend(box_ious.tolist())
        if 'gt_boxes' in r:
            vol = torch.cat(r['gt_boxes'], 0)[:, 3:6].prod(1)
            small.extend(box_ious[vol < 30].tolist())
            medium.extend(box_ious[(vol >= 30) & (vol < 150)].tolist())
            large.extend(box_ious[vol >= 150].tolist())
        total_inter += float(inters.sum())
        total_union += float(unions.sum())
        track.append(float(inters.sum() / unions.sum()))
    if not track:
        return {}
    out = dict(iou=total_inter / total_union, miou_track=sum(track) / len(track), miou_box=sum(box) / len(box))
    for name, lst in (('small', small), ('medium', medium), ('large', large)):
        if lst:
            out['iou_' + name] = sum(lst) / len(lst)
    return out
