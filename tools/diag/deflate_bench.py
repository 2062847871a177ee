"""throughput of the BGZF compressor: sk_bgzf_deflate_dev at level 2 on ~30 MB of gVCF-like text and on one slice of 510 blocks
(device events around each call, after a warm-up), next to zlib levels 1 and 6 on one host core over the same bytes in the same
65 280-byte slices.  usage: python tools/diag/deflate_bench.py [reps] -> one JSON line"""
import ctypes as C
import json
import statistics
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
from tests.test_bgzf_deflate import CUT, _text, _zlib_walk  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
capi.init(0)
L = capi.lib()
SLICE_BLOCKS = 510
pieces, size, seed = [], 0, 1000
while size < SLICE_BLOCKS * CUT:  # the text fixture again and again, a new seed each time
    pieces.append(_text(300000, seed))
    size += len(pieces[-1])
    seed += 1
whole = b"".join(pieces)[:SLICE_BLOCKS * CUT]
inputs = {"text_30MB": whole[:30 * 1000 * 1000], "slice_510_blocks": whole}
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
result = {}


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


for name, data in inputs.items():
    n_blocks = -(-len(data) // CUT)
    cap = capi.bgzf_deflate_bound(len(data), True)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_end = torch.empty(n_blocks + 1, dtype=torch.int64, device="cuda")
    row = dict(bytes=len(data), blocks=n_blocks)
    for level in (2, 1, 0):
        def run():
            capi._check(L.sk_bgzf_deflate_dev(C.c_void_p(d_in.data_ptr()), len(data), level, 1, C.c_void_p(d_out.data_ptr()), cap,
                                              C.c_void_p(d_end.data_ptr()), st))
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps if level == 2 else max(reps // 4, 3)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        total = int(d_end[-1].item())
        if level == 2:
            assert b"".join(_zlib_walk(d_out[:total].cpu().numpy().tobytes())) == data
        row["level%d" % level] = dict(ms=spread(ms), GBps_in=len(data) / statistics.median(ms) / 1e6, out_bytes=total)
    result[name] = row

data = inputs["text_30MB"]
for zl in (1, 6):
    secs, out = [], 0
    for _ in range(3):
        t0 = time.perf_counter()
        out = 0
        for i in range(0, len(data), CUT):
            c = zlib.compressobj(level=zl, wbits=-15)
            out += len(c.compress(data[i:i + CUT]) + c.flush()) + 26
        secs.append(time.perf_counter() - t0)
    result["zlib_level%d_one_core" % zl] = dict(s=spread(secs), GBps_in=len(data) / statistics.median(secs) / 1e9, out_bytes=out + 28)
print(json.dumps(result))
