"""Times the chunked global_ec's two kernels at the production size (profiles/globalec_kernels.txt): a 1' ice grid
(21600 x 10800, 233 M cells) onto the 1/2 deg ocean grid, planes resident in HBM.

  globalec_times.py [reps]      the scan as a whole (host clock around IceScan: regrid, scan, masked counts, their prefix sums,
                                one read-back) and chunk_mask (device events around `reps` launches after a warm-up)

Run it under rocprofv3 --kernel-trace --stats for the kernels on their own (k_gec_scan, k_gec_mask).  Bytes: the scan reads
4 bytes per ice-grid cell at most (the elevation piece only where a piece holds ice), the mask reads 4 and writes 8.  The
yardstick is what this box gives a plain read stream, 5.96 TB/s (roofline.measured_streams)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from icebin_amd import HntrSpec, global_ec  # noqa: E402

READ_STREAM = 5.96e12
O, I = HntrSpec(720, 360, 0., 30.), HntrSpec(21600, 10800, 0., 1.)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def planes(case, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    el = torch.randint(-400, 4000, (I.jm, I.im), dtype=torch.int16, device=dev, generator=g)
    if case == "half":          # every second cell, at random: every 16-byte piece holds ice
        fg = (torch.rand((I.jm, I.im), device=dev, generator=g) < 0.5).to(torch.int16)
    else:                       # two polar caps, 12 % of the rows: most pieces hold none
        fg = torch.zeros((I.jm, I.im), dtype=torch.int16, device=dev)
        fg[:I.jm * 8 // 100] = 1
        fg[-I.jm * 4 // 100:] = 1
    return fg, el


def main(reps=5):
    dev = torch.device("cuda:0")
    for case in ("half", "caps"):
        fg, el = planes(case, dev)
        scan = global_ec.IceScan(O, I, fg, el)              # warm-up: the allocations
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            scan = global_ec.IceScan(O, I, fg, el)
            t.append((time.perf_counter() - t0) * 1e3)
        chunks = scan.chunks()
        out = scan.chunk_mask(chunks[0])
        torch.cuda.synchronize()
        ms = timed(lambda: scan.chunk_mask(chunks[0], out=out), reps)
        nI = I.size
        print(json.dumps(dict(case=case, ice_cells=int(scan.nice.sum()), chunks=len(chunks), scan_create_wall_ms=round(min(t), 3),
                              scan_bytes_max=4 * nI, scan_floor_ms=round(4 * nI / READ_STREAM * 1e3, 4), mask_ms=round(ms, 4),
                              mask_bytes=12 * nI, mask_TBps=round(12 * nI / ms / 1e9, 3),
                              mask_share_of_read_stream=round(12 * nI / READ_STREAM / (ms * 1e-3), 3))), flush=True)
        del scan, out, fg, el


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
