"""The ``bwds_save`` option and its read-only ``last.bwds_save`` on the host (no device): default, accepted and refused values, the
environment variable that seeds it.  One fresh process per case, as in tests/test_gns_api_host.py: options are process-wide."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = dict(HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', GNS_NO_AUTOBUILD='1')


def _child():
    sys.path.insert(0, ROOT)
    import opf_graph_neural_solver_amd as amd
    lib = amd.load_library()
    out = {'seeded': amd.get_option('bwds_save'), 'last': amd.get_option('last.bwds_save'), 'set': []}
    for v in (0, 1, -1, 2):
        out['set'].append([v, lib.gns_set_option(b'bwds_save', v), amd.get_option('bwds_save')])
    out['set last'] = lib.gns_set_option(b'last.bwds_save', 1)
    out['mode untouched'] = amd.get_option('bwds_mode')
    print('RESULT ' + json.dumps(out))


def _run(env=None):
    keep = {k: v for k, v in os.environ.items() if not k.startswith('GNS_') or k == 'GNS_LIB'}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(keep, **NO_DEVICE, **(env or {})))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    assert r.returncode == 0 and len(lines) == 1, r.stdout + r.stderr
    return json.loads(lines[0][len('RESULT '):])


def test_default_values_and_read_only_last():
    o = _run()
    assert o['seeded'] == 1 and o['last'] == -1, o                  # on by default; nothing launched yet
    einval = o['set'][2][1]
    assert einval != 0
    assert o['set'] == [[0, 0, 0], [1, 0, 1], [-1, einval, 1], [2, einval, 1]], o    # 0 and 1 stored; anything else refused, value kept
    assert o['set last'] == einval, o                               # "last.*" names are read-only
    assert o['mode untouched'] == 1, o


@pytest.mark.parametrize('text,value', [('0', 0), ('1', 1), ('2', 1), ('-1', 1)])
def test_environment_seeds_it(text, value):
    assert _run(dict(GNS_BWDS_SAVE=text))['seeded'] == value        # out of range: ignored, the default stays


if __name__ == '__main__':
    _child()
