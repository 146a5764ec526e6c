#!/usr/bin/env python3
"""Exposed LDS waits of a kernel listing (`make -C nerf-cuda_amd asm` -> build/*.s).

An *exposed LDS wait* is an `s_waitcnt lgkmcnt(N)` whose youngest retired operation is a `ds_read*` issued at most WINDOW (8)
instructions earlier: the wave parks for most of an LDS round trip with nothing of its own in between.  The LGKM counter is
modelled in order -- LDS operations and scalar-memory loads enter a queue, a wait for N retires all but the youngest N -- and the
queue is emptied at every label (what is in flight at a join is not known from the text).

Usage: scripts/lds_wait_listing.py build/nrf_kernels_hot_qqfh.s [symbol filter (substring of the demangled or mangled name)]
Per matching symbol: the count over the whole function, the count inside the first two-tile network pass, and a compact trace of
that pass -- L vector-memory load, d ds_read, w ds_write, s scalar load, M MFMA, [lN] / [vN] waits for lgkmcnt / vmcnt (a combined
wait prints both), `!` behind an exposed wait, `.` anything else; a label starts a new line."""
import re
import subprocess
import sys

WINDOW = 8
_LABEL = re.compile(r"^([.\w$@]+):")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")
_VM = re.compile(r"vmcnt\((\d+)\)")


def instructions(lines):
    """[(kind, text)]: kind 'label' or 'inst'; directives, comments and blank lines are dropped"""
    out = []
    for ln in lines:
        s = ln.split(";", 1)[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            out.append(("label", m.group(1)))
            continue
        if s.startswith("."):
            continue
        out.append(("inst", s))
    return out


def _lgkm_kind(op):
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_"):
        return "ds_other"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    return None


def exposed_lds_waits(lines, window=WINDOW):
    """Instruction numbers (labels not counted) of the exposed LDS waits of one function's listing lines."""
    queue, found, n = [], [], 0
    for kind, text in instructions(lines):
        if kind == "label":
            queue = []
            continue
        n += 1
        op = text.split()[0]
        k = _lgkm_kind(op)
        if k:
            queue.append((k, n))
        elif op == "s_waitcnt":
            m = _LGKM.search(text)
            if m is None:
                continue
            keep = int(m.group(1))
            if len(queue) > keep:
                retired, queue = queue[:len(queue) - keep], queue[len(queue) - keep:]
                yk, yn = retired[-1]
                if yk == "ds_read" and n - yn <= window:
                    found.append(n)
    return found


def functions(text, filt=""):
    """{symbol: listing lines} of the functions whose mangled or demangled name contains filt"""
    lines = text.splitlines()
    out, cur, name = {}, None, None
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
            else:
                cur.append(ln)
    if not filt:
        return out
    keep = {}
    for k, v in out.items():
        dem = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        if filt in k or filt in dem:
            keep[k] = v
    return keep


def network_pass(lines, tiles=2, window=WINDOW):
    """(trace, exposed waits inside) of the first network pass: from ahead of the gathers of `tiles` tiles to the last MFMA"""
    ins = instructions(lines)
    exposed = set(exposed_lds_waits(lines, window))
    num, n = [], 0
    for kind, _ in ins:
        n += kind == "inst"
        num.append(n)
    ops = [t.split()[0] if k == "inst" else "" for k, t in ins]
    mf = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
    if not mf:
        return "", 0
    end = mf[0]
    for i in mf[1:]:
        if i - end > 200:
            break
        end = i
    loads = [i for i, o in enumerate(ops[:mf[0]]) if o.startswith(("buffer_load", "global_load", "flat_load"))]
    start, clusters = mf[0], 0
    for i in reversed(loads):
        if start - i > 150:
            clusters += 1
            if clusters > tiles:
                break
        start = i
    start = max(0, start - 40)
    out, inside = [], 0
    for i in range(start, end + 1):
        kind, text = ins[i]
        if kind == "label":
            out.append("\n" + text + ": ")
            continue
        o = ops[i]
        if o.startswith(("buffer_load", "global_load", "flat_load")):
            out.append("L")
        elif o.startswith(("ds_read", "ds_load")):
            out.append("d")
        elif o.startswith("ds_"):
            out.append("w")
        elif _lgkm_kind(o) == "smem":
            out.append("s")
        elif o.startswith("v_mfma"):
            out.append("M")
        elif o == "s_waitcnt":
            l, v = _LGKM.search(text), _VM.search(text)
            mark = "!" if num[i] in exposed else ""
            inside += bool(mark)
            out.append("[" + ("v" + v.group(1) if v else "") + ("l" + l.group(1) if l else "") + "]" + mark)
        else:
            out.append(".")
    return "".join(out).strip(), inside


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    text = open(argv[1]).read()
    for sym, lines in functions(text, argv[2] if len(argv) > 2 else "").items():
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().split("(")[0]
        trace, inside = network_pass(lines)
        print(f"{dem}\n  exposed LDS waits: {len(exposed_lds_waits(lines))} in the function, {inside} in the first two-tile pass")
        if trace:
            print("  " + trace.replace("\n", "\n  "))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
