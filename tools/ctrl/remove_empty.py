#!/usr/bin/env python3
"""Empty-box removal of the CTRL recipe -- command line of the reference's tools/ctrl/remove_empty.py:
    python tools/ctrl/remove_empty.py --bin-path RESULT.bin --split training|testing [--process N] [--type vehicle]
                                      [--gt-bin GT.bin] [--mm-data-root DIR]
Writes <stem>_wo_empty_right.bin next to the input; with --gt-bin the native Waymo table of the result is printed and
written next to it (objectcentricocccompletion_amd/ctrl_prep.py: remove_empty)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--bin-path', type=str, required=True)
    parser.add_argument('--split', type=str, default='training', help='training (train and validation set) or testing')
    parser.add_argument('--process', type=int, default=1)
    parser.add_argument('--type', type=str, default='vehicle', choices=['vehicle', 'pedestrian', 'cyclist'])
    parser.add_argument('--gt-bin', type=str, default=None)
    parser.add_argument('--mm-data-root', type=str, default=None, help='default ./data/waymo/kitti_format')
    args = parser.parse_args(argv)
    from objectcentricocccompletion_amd import ctrl_prep
    if not 1 <= args.process <= ctrl_prep.MAX_PROCESSES:
        parser.error(f'--process {args.process}: between 1 and {ctrl_prep.MAX_PROCESSES} processes may share the GPUs')
    ctrl_prep.remove_empty(args.bin_path, args.split, args.type, args.process, args.gt_bin, mm_data_root=args.mm_data_root)


if __name__ == '__main__':
    main()
