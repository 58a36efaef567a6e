#!/usr/bin/env python
"""Compile reference binaries that tests load, from a checkout of the reference project.

The extension-library tests (tests/test_library_graph.py) drive ``mx.library.load`` with the
reference's own example library ``example/extensions/lib_subgraph/subgraph_lib.cc``, built against
its ``include/mxnet/lib_api.h`` and ``src/lib_api.cc``.  None of that source is part of this
repository: this recipe compiles it where a reference checkout is available and leaves the shared
library in ``oracle/_ref/`` (git-ignored).  Without a checkout nothing is built and those tests skip.

The checkout is looked for in ``$MXAMD_REFERENCE_DIR``, then in ``reference/`` next to this repository.

Usage: ``python oracle/build_ref.py`` (also run by ``__graft_entry__.build()``).
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'oracle', '_ref')

# (output name, sources relative to the reference checkout)
LIBS = [
    ('libsubgraph_lib.so', ['example/extensions/lib_subgraph/subgraph_lib.cc', 'src/lib_api.cc']),
]


def reference_dir():
    cands = [os.environ.get('MXAMD_REFERENCE_DIR'), os.path.join(os.path.dirname(ROOT), 'reference')]
    for d in cands:
        if d and os.path.exists(os.path.join(d, 'include', 'mxnet', 'lib_api.h')):
            return d
    return None


def lib_path(name):
    return os.path.join(OUT, name)


def build():
    ref = reference_dir()
    if ref is None:
        print('oracle: no reference checkout found; reference binaries not built')
        return []
    os.makedirs(OUT, exist_ok=True)
    built = []
    for name, rel in LIBS:
        srcs = [os.path.join(ref, r) for r in rel]
        if not all(os.path.exists(s) for s in srcs):
            print('oracle: %s: sources missing in %s; skipped' % (name, ref))
            continue
        out = lib_path(name)
        if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
            tmp = out + '.tmp%d' % os.getpid()
            subprocess.check_call(['g++', '-shared', '-fPIC', '-O1', '-std=c++17', '-I' + os.path.join(ref, 'include')]
                                  + srcs + ['-o', tmp])
            os.replace(tmp, out)
        built.append(out)
    return built


if __name__ == '__main__':
    for p in build():
        print('built', p)
    sys.exit(0)
