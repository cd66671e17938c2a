#!/usr/bin/env python3
"""Track extension of the CTRL recipe -- command line of the reference's tools/ctrl/extend_tracks.py:
    python tools/ctrl/extend_tracks.py CONFIG
CONFIG is a YAML file of the shape of tools/ctrl/data_configs/extend.yaml (bin_path, direction, extend_length,
min_length_to_extend, score_multiplier, velo_window_size; optional extend_all, min_length_to_extend_all, mm_data_root,
poses_path).  Writes <bin stem>_<config name>.bin next to the input
(objectcentricocccompletion_amd/ctrl_prep.py: extend_tracks)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('config', type=str)
    args = parser.parse_args(argv)
    from objectcentricocccompletion_amd import ctrl_prep
    ctrl_prep.extend_tracks(args.config)


if __name__ == '__main__':
    main()
