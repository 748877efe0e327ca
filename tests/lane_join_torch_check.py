"""Child process of tests/test_lane_join.py::test_caller_on_the_stream_sees_both_halves: torch first (it brings its own HIP
runtime), then the library.  For a context whose stream has been read and for one created on a borrowed torch stream: run()
on 65 pairs whose first half is empty, then at once a torch copy on that stream of the batch's device records; the copy holds
the finished records of both halves -- the same bytes as a one-stream context's download.  Prints '<case> ok' per case."""
import os
import sys

import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvslam_amd import capi, synth  # noqa: E402

P, N, H = 65, 256, 2048
HALF = (P + 1) // 2


class DevBytes:
    """device memory of the library as a torch tensor (the CUDA array interface)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = dict(shape=(nbytes,), typestr="|u1", data=(ptr, False), version=2)


def main():
    d = synth.make_batch(700, P, n_kp=N)
    n1, n2 = d["n1"].copy(), d["n2"].copy()
    n1[:HALF], n2[:HALF] = 0, 0   # every record that counts is the second half's, the main lane is idle at once
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=91, max_error_sq=1e-2)

    def batch(ctx):
        b = capi.Batch(ctx, P, N, 32)
        b.upload(0, d["desc1"], d["kp1"], n1, d["desc2"], d["kp2"], n2, d["K"], d["global_index"])
        return b

    off = capi.Context(0)
    off.set_half_batches(False)
    b = batch(off)
    b.run(prm)
    want = b.download(matches=False, mask=False, points=False)["results"]
    b.close()
    off.close()
    assert int(want["n_matches"][HALF:].sum()) > 0 and int(want["valid"][HALF:].sum()) > 0

    for how in ("stream_read", "borrowed"):
        if how == "borrowed":
            ts = torch.cuda.Stream()
            ctx = capi.Context(0, stream=ts.cuda_stream)
        else:
            ctx = capi.Context(0)
            ts = torch.cuda.ExternalStream(ctx.stream)
        b = batch(ctx)
        ptr, rec_bytes = b.results_device()   # the records' address and the size of one
        nbytes = P * rec_bytes
        b.run(prm)
        with torch.cuda.stream(ts):   # whether torch aliases the records or copies them at once: it reads them on ts
            seen = torch.as_tensor(DevBytes(ptr, nbytes), device="cuda:0").clone()
        ts.synchronize()
        got = seen.cpu().numpy().tobytes()[:want.nbytes]
        b.close()
        ctx.close()
        if got != want.tobytes():
            rec = want.itemsize
            bad = [i for i in range(P) if got[i * rec:(i + 1) * rec] != want[i].tobytes()]
            print("%s: the copy on the caller's stream differs from the one-stream records in pairs %s" % (how, bad))
            return 1
        print("%s ok" % how)
    return 0


if __name__ == "__main__":
    sys.exit(main())
