"""Generate tests/golden/ococcnet_model_cfg.pkl: the ``model`` dict of the REFERENCE's configs/ococc/ococcnet.py as plain
python evaluates it -- before any loader rebuilds it, so the pickle keeps the lists that ``[[16, 32]] * 6`` and its like
share between blocks.  Data only, no reference source: dicts, lists, tuples, numbers and strings."""
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from objectcentricocccompletion_amd import config  # noqa: E402

REF = os.environ.get('OCOCC_REFERENCE', '/root/reference')


def main():
    model = config._load_py(os.path.join(REF, 'configs', 'ococc', 'ococcnet.py'))['model']
    path = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'ococcnet_model_cfg.pkl')
    with open(path, 'wb') as f:
        pickle.dump(model, f, protocol=4)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
