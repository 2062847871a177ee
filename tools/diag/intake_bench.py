"""time of the read intake: sk_read_intake_dev (device events around each call, after a warm-up) on one pileup-stream window
(2 200 reads x 150 bp) and on 2^20 reads x 150 bp at ~40x, the arrays resident on the device as the feed leaves them.
The window's result is checked against the model (tests/intake_model.py); the large shape is the window's reads tiled over a periodic
reference, checked tile against tile.  usage: python tools/diag/intake_bench.py [reps] -> one JSON line"""
import ctypes as C
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from strelka_amd import capi  # noqa: E402
from tests import intake_cases as K  # noqa: E402
from tests import intake_model as M  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
capi.init(0)
L = capi.lib()
READ_LEN, DEPTH = 150, 40
POOL = 2200
CHUNK = POOL * READ_LEN // DEPTH  # reference positions one pool of reads covers at DEPTH
OFF = 1000


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


# a pool of reads over one period of a periodic reference (a read that runs past the period's end continues into the next, identical one)
rng = np.random.default_rng(8801)
period = K.repeat_rich_reference(CHUNK, rng)
starts = np.sort(rng.integers(OFF, OFF + CHUNK, POOL))
pool = [K.random_read(period * 3, OFF, int(s), READ_LEN, rng) for s in starts]
pool, pool_low = K.usable(pool, [int(x) for x in rng.random(POOL) < 0.05])
read_off, code, path_off, n_seg, path, pos = capi.pack_reads(pool)
n_pool = len(pool)


def tiled(tiles):
    """the pool `tiles` times, each copy one period further -> the arrays sk_read_intake_dev takes, and the window"""
    n = n_pool * tiles
    lens = np.tile(np.diff(read_off), tiles)
    segs = np.tile(np.diff(path_off), tiles)
    arrays = dict(read_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), code=np.tile(code[:int(read_off[-1])], tiles),
                  path_off=np.concatenate([[0], np.cumsum(segs)]).astype(np.int64), n_seg=np.tile(n_seg[:n_pool], tiles),
                  path=np.tile(path[:int(path_off[-1])], tiles),
                  pos=(np.tile(pos[:n_pool], tiles).astype(np.int64) + np.repeat(np.arange(tiles, dtype=np.int64) * CHUNK, n_pool)).astype(np.int32),
                  low=np.tile(np.array(pool_low, np.uint8), tiles))
    return n, arrays, OFF - 10, CHUNK * tiles + 2 * READ_LEN + 200


result = {}
for name, tiles in (("window_2200_reads", 1), ("reads_2^20", -(-(1 << 20) // n_pool))):
    n, a, win_begin, n_pos = tiled(tiles)
    ref = period * (tiles + 2)
    d = {k: torch.from_numpy(np.ascontiguousarray(v.view(np.uint32) if k == "path" else v)).cuda() for k, v in a.items()}
    d_ref = torch.from_numpy(np.frombuffer(ref.encode(), np.uint8).copy()).cuda()
    n_segs = int(a["path_off"][-1])
    cap = capi.read_intake_obs_bound(n_segs)
    d_reads = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    d_obs_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_obs = torch.empty(cap * 32, dtype=torch.uint8, device="cuda")
    d_sites = torch.empty(n_pos, dtype=torch.int64, device="cuda")
    d_cand = torch.empty(n_pos, dtype=torch.uint8, device="cuda")
    scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, n_pos)
    d_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device="cuda")
    opt = capi.intake_options()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def run():
        capi._check(L.sk_read_intake_dev(p(d_ref), OFF, len(ref), n, p(d["read_off"]), p(d["code"]), p(d["path_off"]), p(d["n_seg"]), p(d["path"]), p(d["pos"]),
                                         p(d["low"]), C.byref(opt), win_begin, n_pos, p(d_reads), p(d_obs_off), p(d_obs), cap, p(d_sites), p(d_cand),
                                         p(d_scratch), scratch_bytes, st))

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    rec = d_reads.cpu().numpy().view(capi.INTAKE_READ_DTYPE)
    sites = d_sites.cpu().numpy().view(capi.INTAKE_SITE_DTYPE)
    n_obs = int(d_obs_off[-1].item())
    if tiles == 1:
        want = M.read_intake(ref, OFF, pool, pool_low, win_begin, n_pos)
        assert [tuple(int(x) for x in r) for r in rec] == want["reads"]
        assert [tuple(int(x) for x in s) for s in sites] == want["sites"]
        assert d_cand.cpu().numpy().astype(bool).tolist() == want["is_candidate"]
        assert n_obs == len(want["obs"])
    else:  # every tile's reads give the pool's records, every inner period the same counters
        assert (rec.reshape(tiles, n_pool) == rec[:n_pool][None, :]).all()
        inner = sites[10 + CHUNK:10 + CHUNK * (tiles - 1)].reshape(tiles - 2, CHUNK)
        assert (inner == inner[0][None, :]).all()
    n_bases = int(a["read_off"][-1])
    result[name] = dict(reads=n, bases=n_bases, segments=n_segs, positions=n_pos, observations=n_obs, ms=spread(ms),
                        reads_per_us=n / statistics.median(ms) / 1e3)
print(json.dumps(result))
