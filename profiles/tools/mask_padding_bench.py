#!/usr/bin/env python3
"""Cost of mask_padding (hparam; the L1 losses over each utterance's real frames): the `mixed` training step at the
benchmark shape (N 32, T_in 160, T_out 1000) of Tacotron-2 and Tacotron-1 in three configurations - the parent commit
(--parent DIR: a checkout of it with its library built), this commit with the switch off, and this commit with the switch
on and feeder-like lengths (FRAMES below: a length-sorted batch whose shortest utterance has 0.55 of the longest one's
frames, 22 % of the padded batch is padding).

Each tree runs in a worker process of its own (this file with --worker, importing that tree's package and bench.py), which
holds ONE model and one device-resident synthetic batch (bench.synthetic_batch); off and on are the same model with its
`mask_padding` attribute switched between windows, so both run on the same buffers.  The driver never touches the GPU: it
asks the workers for one window at a time - a window is STEPS steps between two device synchronisations - and rotates the
order of the configurations from round to round, so that they alternate in one session and share whatever else the
machine does.  Only one worker works at any time.  Then the two loss launches alone on an otherwise idle chip (device
events around the calls): ns_l1_loss against ns_l1_loss_masked with full and with feeder-like lengths, at the linear
term's shape (F 1025, bf16 gradient) and the mel term's (F 80), with the bytes each moves.
Usage: python profiles/tools/mask_padding_bench.py [--parent DIR] [rounds] [steps per window]"""
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, TI, TO = 32, 160, 1000
HBM_COPY = 6.3e12


def frames():
    import numpy as np
    return np.round(np.linspace(1.0, 0.55, N) * TO).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- worker
def worker(root, name, steps):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bench
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model

    hp = hparams_mod.load(name)
    has_switch = hasattr(hp, "mask_padding")
    batch = bench.synthetic_batch(hp, N, TI, TO, 1234)
    m = create_model(name, hp, device="cuda:0", dtype="mixed", seed=1234)
    m.add_loss().add_optimizer(global_step=0)
    m.initialize(batch[0], batch[1], None, batch[2], batch[3], target_lengths=frames())    # uploads the batch once
    for on in ((False, True) if has_switch else (False,)):
        m.mask_padding = on
        for _ in range(3):
            m.step(read_loss=False)
    torch.cuda.synchronize()
    m.check_status()
    print("ready %d" % int(has_switch), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        if cmd in ("off", "on"):
            m.mask_padding = cmd == "on"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.step(read_loss=False)
            torch.cuda.synchronize()
            print("ms %.6f" % ((time.perf_counter() - t0) / steps * 1e3), flush=True)
        elif cmd == "loss":
            out = []
            for on in (False, True):
                m.mask_padding = on
                m.step(read_loss=False)
                m.read_losses()
                out.append("%s loss %.5f (mel %.5f, linear %.5f) over %d frames"
                           % ("on" if on else "off", m.loss, m.mel_loss, m.linear_loss, m._loss_frames))
            m.check_status()
            print("loss " + "; ".join(out), flush=True)
        elif cmd == "alone":
            del m
            torch.cuda.empty_cache()
            for text in launches_alone(torch, np):
                print("line " + text, flush=True)
            print("done", flush=True)


def launches_alone(torch, np):
    from nspeech_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    fr = frames()
    lens = {"full": None, "feeder-like": torch.from_numpy(fr.astype(np.int32)).to(dev)}
    share = float(fr.sum()) / (N * TO)
    P, padl = TO + 16, 8

    def timed(fn, reps=50):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for what, F, ld, gdt, n_prio in (("linear term", 1025, 1028, torch.bfloat16, 205), ("mel term", 80, 80, torch.float32, 0)):
        pred = torch.randn(N * P * ld, device=dev, generator=g)
        tgt = torch.randn(N * TO * F, device=dev, generator=g)
        dp = torch.zeros(N * P * ld, device=dev, dtype=gdt)
        acc = torch.zeros(8, device=dev)
        work = torch.zeros(ops.l1_loss_masked_work_floats(N, TO, F), device=dev)
        gb = dp.element_size()
        full = N * TO * F * (8 + gb)
        ms = timed(lambda: ops.l1_loss(pred, ld, tgt, dp, ld, N, TO, P, padl, F, n_prio, 1e-6, 1e-6, acc))
        yield ("%s (F %d, %s gradient): ns_l1_loss %.4f ms per call, %.1f MB -> %.0f GB/s = %.0f %% of the 6.3 TB/s copy rate"
               % (what, F, "bf16" if gb == 2 else "fp32", ms, full / 1e6, full / (ms * 1e-3) / 1e9,
                  100.0 * full / (ms * 1e-3) / HBM_COPY))
        for k, ln in lens.items():
            ms = timed(lambda: ops.l1_loss_masked(pred, ld, tgt, dp, ld, N, TO, P, padl, F, n_prio, 1e-6, 1e-6, ln, acc, work))
            real = 1.0 if ln is None else share
            moved = N * TO * F * (8 * real + gb)            # the padded frames are not loaded, their gradient is written
            yield ("%s: ns_l1_loss_masked, %s lengths, %.4f ms per call (two kernels), %.1f MB -> %.0f GB/s = %.0f %%"
                   % (what, k, ms, moved / 1e6, moved / (ms * 1e-3) / 1e9, 100.0 * moved / (ms * 1e-3) / HBM_COPY))


# ---------------------------------------------------------------------------------------------------- driver
class Worker(object):
    def __init__(self, root, name, steps):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, name, str(steps)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        self.has_switch = bool(int(self.expect("ready")))

    def expect(self, word):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError("the worker ended (exit code %s)" % self.p.poll())
            if line.startswith(word + " ") or line.strip() == word:
                return line[len(word):].strip()
            if line.startswith("line "):
                print(line[5:].rstrip(), flush=True)

    def ask(self, cmd, word):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        return self.expect(word)

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait(timeout=120)


def main():
    import numpy as np
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    rounds = int(args[0]) if args else 6
    steps = int(args[1]) if len(args) > 1 else 20
    fr = frames()
    print("# mask_padding: mixed step, N %d, T_in %d, T_out %d; %d rounds of %d steps per configuration; lengths %d .. %d, "
          "%.1f %% of the padded batch is padding" % (N, TI, TO, rounds, steps, fr.max(), fr.min(),
                                                     100.0 * (1.0 - fr.sum() / float(N * TO))))
    for name in ("taco2", "taco1"):
        here = Worker(HERE, name, steps)
        assert here.has_switch
        cfgs = [("off", here, "off"), ("on", here, "on")]
        if parent:
            par = Worker(parent, name, steps)
            assert not par.has_switch, "--parent must be a tree without the switch"
            cfgs.insert(0, ("parent", par, "off"))
        times = {c[0]: [] for c in cfgs}
        for rnd in range(rounds):
            order = cfgs[rnd % len(cfgs):] + cfgs[:rnd % len(cfgs)]             # rotate which one goes first
            for key, w, cmd in order:
                times[key].append(float(w.ask(cmd, "ms")))
            print("%s round %d: %s" % (name, rnd, " | ".join("%s %.3f" % (c[0], times[c[0]][-1]) for c in cfgs)), flush=True)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("%s median ms/step: %s" % (name, " | ".join("%s %.3f (%.3f .. %.3f)" % (k, med[k], min(v), max(v))
                                                         for k, v in times.items())))
        base = "parent" if parent else "off"
        for k in times:
            if k != base:
                print("%s %s against %s: %+.3f ms = %+.2f %%" % (name, k, base, med[k] - med[base],
                                                               100.0 * (med[k] - med[base]) / med[base]))
        print("%s after the run: %s" % (name, here.ask("loss", "loss")), flush=True)
        if parent:
            par.close()
        if name == "taco1":                 # the last worker gives its model up and times the launches alone
            here.ask("alone", "done")
        here.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
