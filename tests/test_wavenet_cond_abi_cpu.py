"""ns_wavenet_generate's condition rows (cond_rows / cond_hold / cond_t0, include/nspeech_hip.h): the host refuses a
call whose steps would read a row that is not there, or a condition on an engine that takes none, before any launch -
so these run without a GPU (the pointers below are never followed)."""
import ctypes

from nspeech_amd import _lib

ERR_ARG = -1


def _params(**over):
    p = _lib.struct("ns_wavenet_generate_params")
    fake = 0x1000                            # non-null; every case here is refused before a kernel could read it
    for f in ("weights", "ids", "queues", "uniform", "dilations"):
        setattr(p, f, fake)
    p.w_dtype = _lib.NS_BF16
    p.L, p.R, p.Dc, p.S, p.Q = 8, 32, 32, 64, 64
    p.B, p.n_seed, p.total, p.queue_rows = 1, 12, 20, 30
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _refused(p):
    lib = _lib.lib()
    rc = lib.ns_wavenet_generate(ctypes.byref(p), None)
    return rc, lib.ns_last_error().decode()


def test_struct_has_the_condition_row_fields():
    p = _lib.struct("ns_wavenet_generate_params")
    fields = dict((f[0], f[1]) for f in p._fields_)
    assert {"cond_rows", "cond_hold", "cond_t0"} <= set(fields)
    assert fields["cond_rows"] is ctypes.c_int and fields["cond_hold"] is ctypes.c_int and fields["cond_t0"] is ctypes.c_int64
    names = [f[0] for f in p._fields_]       # appended: every earlier member keeps its offset
    assert names[-3:] == ["cond_rows", "cond_hold", "cond_t0"] and names[-5:-3] == ["post_x", "helper_stream"]
    assert type(p).cond_rows.offset > type(p).helper_stream.offset


def test_rows_need_a_hold():
    rc, msg = _refused(_params(cond=0x1000, cond_rows=2, cond_hold=0))
    assert rc == ERR_ARG and "cond_hold" in msg


def test_a_row_that_is_not_there_is_refused():
    # positions 0 .. 19 at 4 samples per row end on row 4; cond has rows 0 and 1
    rc, msg = _refused(_params(cond=0x1000, cond_rows=2, cond_hold=4, total=20, cond_t0=0))
    assert rc == ERR_ARG and "row 4" in msg and "2 rows" in msg
    # the same call seen from further left (a seed in front of row 0) still ends on row 2
    rc, msg = _refused(_params(cond=0x1000, cond_rows=2, cond_hold=4, total=20, cond_t0=-11))
    assert rc == ERR_ARG and "row 2" in msg


def test_the_valu_chain_still_takes_no_condition():
    rc, msg = _refused(_params(cond=0x1000, fgT=0x1000, deT=0x1000, engine=1))
    assert rc == ERR_ARG and "conditions / biases" in msg
    rc, msg = _refused(_params(dense_bias=0x1000, fgT=0x1000, deT=0x1000, engine=3))
    assert rc == ERR_ARG and "conditions / biases" in msg


def test_engine_3_no_longer_consults_helper_stream():
    # the helpers are workgroups of the chain's own launch: helper_stream keeps its place in the struct and is ignored.
    # NULL, and the call's own stream, once failed engine 3's precondition; now such a block passes it and a span is
    # refused with the span's message, which stands behind that precondition
    lib = _lib.lib()
    sp = _lib.struct("ns_wavenet_span_params")
    sp.t_begin, sp.t_end, sp.carry = 5, 9, 0x1000
    call_stream = 0x3000                     # never followed: the refusal stands in front of the first enqueue
    for hs in (0, call_stream):
        p = _params(fgT=0x1000, deT=0x1000, engine=3, S=512, Q=256, post_x=0x1000, helper_stream=hs)
        rc = lib.ns_wavenet_generate_span(ctypes.byref(p), None, ctypes.byref(sp), ctypes.c_void_p(call_stream))
        msg = lib.ns_last_error().decode()
        assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_span: engine 3 takes no span"), msg


def test_the_per_layer_kernel_refuses_an_odd_dc():
    # Dc = 1 passes every divisibility check (512 % (2 Dc) == 0), but the kernel's float64 row follows 3 Dc floats in LDS:
    # an odd Dc leaves it 4 bytes off an 8-byte boundary
    rc, msg = _refused(_params(Dc=1, R=32))
    assert rc == ERR_ARG and "even Dc" in msg


def test_chain_fits_follows_the_layer_count():
    lib = _lib.lib()
    # shipped widths: 50 layers fit with and without a condition row; 74 only without (L * 384 bytes more)
    assert lib.ns_wavenet_chain_fits(50, 32, 512, 256, 1) == 1 and lib.ns_wavenet_chain_fits(73, 32, 512, 256, 1) == 1
    assert lib.ns_wavenet_chain_fits(74, 32, 512, 256, 1) == 0 and lib.ns_wavenet_chain_fits(128, 32, 512, 256, 0) == 1
    assert lib.ns_wavenet_chain_fits(0, 32, 512, 256, 0) == 0


def test_conditioned_chain_reports_no_scratch():
    """The chain wave of wn_generate_mfma_kernel<true> has no register to spare, and a scratch access drags a vmcnt(0)
    wait behind its weight prefetches: the compiler's own resource remarks for that instantiation must say zero scratch
    and no VGPR spill, with the flags of the real build."""
    import os
    import re
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    sh = open(os.path.join(csrc, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', sh, re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "wavenet.hip", "-o",
                        os.devnull], cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)
    cond = [b for b in blocks if b.startswith("_Z23wn_generate_mfma_kernelILb1EE")]
    assert len(cond) == 1, [b.split()[0] for b in blocks[1:]]
    assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", cond[0]).group(1) == "0", cond[0]
    assert re.search(r"VGPRs Spill: (\d+)", cond[0]).group(1) == "0", cond[0]
