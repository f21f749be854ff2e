"""Worker for tests/test_gpu_dw_paths.py::test_dw_fast_path_matches_generic (run in a fresh process:
the library reads FSCNN_DW_GENERIC once).  Runs worker_cases() of that file through every form --
forward with and without the lazy input BN, dgrad with BN partials in modes 0 and 2, wgrad with and
without the lazy x BN, the eval forward and the plain dgrad -- and writes every output, BN record
and slab, in a fixed order, as raw bytes after a one-line header each.  Prints one JSON line: the
compile-time chunk width each case's tile launches take (fscnn_dw3x3_ct_width; 0 = the generic
kernels).

    python tests/_dw_paths_worker.py OUT.bin
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import _lib
    import test_gpu_dw_paths as t

    widths = []
    with open(out, "wb") as f:
        def put(tag, o):
            for k in sorted(o):
                v = o[k].detach().cpu().contiguous()
                f.write(("%s.%s %s %s\n" % (tag, k, v.dtype, tuple(v.shape))).encode())
                f.write(v.reshape(-1).view(torch.uint8).numpy().tobytes())

        for case in t.worker_cases():
            dt, stride, H, W, C = case
            widths.append(_lib.load().fscnn_dw3x3_ct_width(t.N, H, W, C, stride, _lib.dtype_code(dt)))
            for lazy in (1, 0):
                put("%s fwd_train lazy%d" % (t.cid(case), lazy), t.run_fwd_train(dt, stride, H, W, C, lazy)[1])
                put("%s wgrad lazy%d" % (t.cid(case), lazy), t.run_wgrad(dt, stride, H, W, C, lazy)[1])
            for mode in (0, 2):
                put("%s dgrad_bn mode%d" % (t.cid(case), mode), t.run_dgrad_bn(dt, stride, H, W, C, mode)[1])
            put("%s plain" % t.cid(case), t.run_plain(dt, stride, H, W, C)[1])
    print(json.dumps({"widths": widths}))


if __name__ == "__main__":
    main(sys.argv[1])
