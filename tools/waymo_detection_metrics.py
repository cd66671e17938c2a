#!/usr/bin/env python
"""Waymo detection metrics of a result file, natively: the argv shape of compute_detection_metrics_main,

    tools/waymo_detection_metrics.py PRED.bin GT.bin [--assume-points] [--matcher {score_first,hungarian}]

prints the OBJECT_TYPE / RANGE table in the tool's layout, so that it can stand in for it:
``tools/test.py ... --eval waymo --eval-options metrics_main=tools/waymo_detection_metrics.py``.
Box overlap and matching run on the HIP kernels (objectcentricocccompletion_amd/waymo_metrics.py, which states the
protocol).  KNOWN DEPARTURES from the official tool: a score-first greedy matcher instead of its default Hungarian one,
and no recall-delta point insertion; the difference to the official numbers has not been measured.
--matcher hungarian: per score cutoff the matching of maximum total overlap (DESIGN 3.10 rule 4b, our reading of the tool's
default matcher) instead of the score-first one; the second departure stays.
--assume-points: ground-truth files without lidar point counts (everything would be "ignored"): take a missing count
as LEVEL_1."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('pred_bin', help='metrics.Objects file of the predictions')
    ap.add_argument('gt_bin', help='metrics.Objects file of the ground truth')
    ap.add_argument('--assume-points', action='store_true', help='a missing lidar point count is LEVEL_1')
    ap.add_argument('--matcher', choices=('score_first', 'hungarian'), default='score_first',
                    help='score_first (default): greedy by score; hungarian: maximum total overlap per score cutoff')
    a = ap.parse_args(argv)
    from objectcentricocccompletion_amd import waymo_metrics
    return waymo_metrics.evaluate_files(a.pred_bin, a.gt_bin, a.assume_points, matcher=a.matcher)


if __name__ == '__main__':
    main()
