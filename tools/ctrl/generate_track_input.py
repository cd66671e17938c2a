#!/usr/bin/env python3
"""Step 4 of the tracklet data preparation -- command line of the reference's tools/ctrl/generate_track_input.py:
    python tools/ctrl/generate_track_input.py CONFIG [--process N]
CONFIG is a YAML file of tools/ctrl/data_configs (the reference's files are read unchanged; ``mm_data_root`` is an
optional extra key).  Writes <data_root>/<config name>_<split>_database/*.npy and <data_root>/<config name>_<split>.pkl
(objectcentricocccompletion_amd/ctrl_prep.py: generate_track_input)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('config', type=str)
    parser.add_argument('--process', type=int, default=1)
    args = parser.parse_args(argv)
    from objectcentricocccompletion_amd import ctrl_prep
    if not 1 <= args.process <= ctrl_prep.MAX_PROCESSES:
        parser.error(f'--process {args.process}: between 1 and {ctrl_prep.MAX_PROCESSES} processes may share the GPUs')
    ctrl_prep.generate_track_input(args.config, args.process)


if __name__ == '__main__':
    main()
