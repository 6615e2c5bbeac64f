#!/usr/bin/env python
"""Run the reference's own unit tests of the analytics, seen-node and device hooks, read in place, against ``tgm_amd`` (``import tgm``
resolves to ``tgm_amd`` through replay_reference_tests.alias_package).  Its own process: the aliasing rewrites ``sys.modules``.

    python tests/golden/replay_reference_hooks_extra.py      # exit code 0 when every case passes; 77 when there is no reference checkout
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('TGM_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
TEST_DIR = os.path.join(REFERENCE, 'test', 'unit', 'test_hooks')
FILES = ['test_batch_analytics_hook.py', 'test_node_analytics_hook.py', 'test_seen_nodes_track_hook.py', 'test_device_transfer_hook.py',
         'test_pin_memory_hook.py']  # fmt: skip


def main() -> int:
    paths = [os.path.join(TEST_DIR, f) for f in FILES]
    if not all(os.path.exists(p) for p in paths):
        print(f'[replay] no reference checkout at {REFERENCE}')
        return 77
    import pytest

    sys.path.insert(0, HERE)
    from replay_reference_tests import _Tally, alias_package

    alias_package()
    tally = _Tally()
    rc = pytest.main(['-p', 'no:cacheprovider', '-o', 'addopts=', '-c', os.devnull, '--rootdir', TEST_DIR, '-q', '-m', 'not gpu', '-W', 'ignore', *paths],
                     plugins=[tally])  # fmt: skip
    print(f'[replay] {", ".join(FILES)} against tgm_amd: {tally.passed} / {tally.passed + len(tally.failed)}', flush=True)
    for f in tally.failed:
        print(f'[replay] FAILED {f}', flush=True)
    return 0 if (rc == 0 and not tally.failed and tally.passed > 0) else 1


if __name__ == '__main__':
    sys.exit(main())
