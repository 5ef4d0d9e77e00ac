"""CPU: the demultiplexing entries of include/seeq_amd.h (seeqdevScanRunDemux ...) -- record layout, exports, and the
argument checks, which run before any device call and so fail the same way without a GPU."""
import ctypes as C
import errno
import os
import re

import numpy as np

from conftest import ROOT


def test_demux_record_layout(capi):
    # seeqdev_demux_t: 16 bytes, the fields where seeq_amd.h puts them (and where device.DEMUX_DTYPE reads them)
    from seeq_amd import device as dev
    T = capi.seeqdev_demux_t
    assert C.sizeof(T) == 16
    assert [(n, getattr(T, n).offset) for n in ("line", "start", "end", "dist", "pattern", "margin")] == \
        [("line", 0), ("start", 4), ("end", 8), ("dist", 12), ("pattern", 14), ("margin", 15)]
    assert C.sizeof(capi.seeqdev_demux_counts_t) == 24
    assert dev.DEMUX_DTYPE.itemsize == 16
    assert [dev.DEMUX_DTYPE.fields[n][1] for n in ("line", "start", "end", "dist", "pattern", "margin")] == [0, 4, 8, 12, 14, 15]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seeq_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} seeqdev_demux_t;", src).group(1)
    assert re.findall(r"(uint\d+_t)\s+(\w+);", body) == [("uint32_t", "line"), ("uint32_t", "start"), ("uint32_t", "end"),
                                                         ("uint16_t", "dist"), ("uint8_t", "pattern"), ("uint8_t", "margin")]


def test_demux_symbols_exported(capi):
    L = capi.lib()
    for name in ("seeqdevScanRunDemux", "seeqdevScanHostDemux", "seeqdevScanDemuxDevice", "seeqdevScanCopyDemux"):
        assert name in capi.EXPORTS
        assert hasattr(L, name), name


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_demux_argument_checks_without_a_device(capi):
    # The checks come before the context or a pattern is touched: stand-in addresses are never dereferenced.
    L = capi.lib()
    ctx = C.create_string_buffer(4096)
    fake = [C.create_string_buffer(64) for _ in range(256)]
    pats = (C.c_void_p * 256)(*[C.addressof(b) for b in fake])
    text = b"ACGT\n"
    cnt = capi.seeqdev_demux_counts_t()
    per = (C.c_uint64 * 256)()
    run = L.seeqdevScanHostDemux
    _einval(lambda: run(C.addressof(ctx), pats, 0, text, len(text), 0, C.byref(cnt), per))            # npat 0
    _einval(lambda: run(C.addressof(ctx), pats, 256, text, len(text), 0, C.byref(cnt), per))          # npat 256
    _einval(lambda: run(C.addressof(ctx), None, 2, text, len(text), 0, C.byref(cnt), per))            # NULL pats
    _einval(lambda: run(C.addressof(ctx), pats, 2, text, len(text), capi.SQ_ALL, C.byref(cnt), per))  # SQ_ALL
    _einval(lambda: run(C.addressof(ctx), pats, 2, text, len(text), capi.SQ_COUNT, C.byref(cnt), per))
    _einval(lambda: run(None, pats, 2, text, len(text), 0, C.byref(cnt), per))                        # NULL context
    _einval(lambda: run(C.addressof(ctx), pats, 2, text, len(text), 0, None, per))                    # NULL counts
    _einval(lambda: run(C.addressof(ctx), pats, 2, None, 5, 0, C.byref(cnt), per))                    # NULL text
    with_null = (C.c_void_p * 2)(C.addressof(fake[0]), None)
    _einval(lambda: L.seeqdevScanHostDemux(C.addressof(ctx), with_null, 2, text, len(text), 0, C.byref(cnt), per))
    _einval(lambda: L.seeqdevScanRunDemux(C.addressof(ctx), pats, 0, None, 0, 0, C.byref(cnt), per))
    _einval(lambda: L.seeqdevScanRunDemux(C.addressof(ctx), pats, 256, None, 0, 0, C.byref(cnt), per))
    _einval(lambda: L.seeqdevScanRunDemux(C.addressof(ctx), None, 1, None, 0, 0, C.byref(cnt), per))
    _einval(lambda: L.seeqdevScanRunDemux(C.addressof(ctx), pats, 1, None, 0, capi.SQ_ALL, C.byref(cnt), per))
    _einval(lambda: L.seeqdevScanRunDemux(C.addressof(ctx), pats, 1, None, 16, 0, C.byref(cnt), per))
    # no context: no records to copy, no device pointer
    out = np.zeros(1, dtype=np.uint8)
    _einval(lambda: L.seeqdevScanCopyDemux(None, out.ctypes.data, 0, 1))
    assert L.seeqdevScanDemuxDevice(None) is None
