#!/usr/bin/env python
"""Run the reference's own test/unit/test_hooks/test_tgb_negative_sampling_hook.py and test_recipe.py, read in place, against ``tgm_amd``
(``import tgm`` resolves to ``tgm_amd`` through replay_reference_tests.alias_package), with ``tgb`` importable: the installed package, else
the stand-in under tests/golden/_tgb_stub.  Its own process: the aliasing rewrites ``sys.modules``.

    python tests/golden/replay_reference_tgbneg.py      # exit code 0 when every case passes; 77 when there is no reference checkout
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
TEST_DIR = os.path.join(REFERENCE, 'test', 'unit', 'test_hooks')
TEST_FILES = [os.path.join(TEST_DIR, f) for f in ('test_tgb_negative_sampling_hook.py', 'test_recipe.py')]


def main() -> int:
    if not all(os.path.exists(f) for f in TEST_FILES):
        print(f'[replay] no reference checkout at {REFERENCE}')
        return 77
    import pytest

    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    from replay_reference_tests import _Tally, alias_package

    alias_package()
    import tgbneg_cases

    tgbneg_cases.ensure_tgb()
    tally = _Tally()
    rc = pytest.main(['-p', 'no:cacheprovider', '-o', 'addopts=', '-c', os.devnull, '--rootdir', TEST_DIR, '-q', '-m', 'not gpu', '-W', 'ignore',
                      *TEST_FILES], plugins=[tally])  # fmt: skip
    print(f'[replay] test_tgb_negative_sampling_hook.py, test_recipe.py against tgm_amd: {tally.passed} / {tally.passed + len(tally.failed)}', flush=True)
    for f in tally.failed:
        print(f'[replay] FAILED {f}', flush=True)
    return 0 if (rc == 0 and not tally.failed and tally.passed > 0) else 1


if __name__ == '__main__':
    sys.exit(main())
