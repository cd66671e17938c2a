#!/usr/bin/env python3
"""Step 5 of the tracklet data preparation -- command line of the reference's tools/ctrl/generate_candidates.py:
    python tools/ctrl/generate_candidates.py CONFIG [--gt-bin-path P] [--process N]
Reads <data_root>/<config name>_<split>.pkl (step 4) and the ground-truth .bin (``gt.bin`` in place of ``train_gt.bin``
for the val split), writes <data_root>/<config name>_<split>_gt_candidates.pkl
(objectcentricocccompletion_amd/ctrl_prep.py: generate_candidates)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('config', type=str)
    parser.add_argument('--gt-bin-path', type=str, default='./data/waymo/waymo_format/train_gt.bin')
    parser.add_argument('--process', type=int, default=1)
    args = parser.parse_args(argv)
    from objectcentricocccompletion_amd import ctrl_prep
    if not 1 <= args.process <= ctrl_prep.MAX_PROCESSES:
        parser.error(f'--process {args.process}: between 1 and {ctrl_prep.MAX_PROCESSES} processes may share the GPUs')
    beg = time.time()
    ctrl_prep.generate_candidates(args.config, args.gt_bin_path, args.process)
    print(f'Time cost: {time.time() - beg} seconds.')


if __name__ == '__main__':
    main()
