"""Instruction mix of kernels matching a regex in a hipcc -S dump: tools/isamix.py REGEX [asmfile] [--loop] [--dpp-hazards]

--loop         count the kernel's hottest loop instead of the whole function: from the last loop-header label ahead of the
               function's last MFMA to the branch back to it (the step loop of the fused passes); also lists the loop's
               s_waitcnt vmcnt immediates in program order.
--dpp-hazards  report every DPP instruction whose DPP source (src0) is written by a vector instruction within the two
               instructions before it.  Inline-assembly DPP (TEHMM_TAIL_FMA) gets no hazard nops from the compiler, so
               the count must be 0 for the kernels that use it; exit status 1 otherwise.
"""
import re, subprocess, sys
from collections import Counter

flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
asm = args[1] if len(args) > 1 else "/tmp/lane.s"
if len(args) <= 1:
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
                    "-I/root/repo/include", "-S", "--cuda-device-only", "/root/repo/tehmm_amd/csrc/tehmm_hip.hip",
                    "-o", asm], check=True, stderr=subprocess.DEVNULL)
s = open(asm).read()
pat = re.compile(args[0])


def is_instr(l):
    t = l.strip()
    return bool(t) and not t.startswith((';', '.')) and not t.endswith(':') and not re.match(r'\.?\w+:', t)


def vregs(tok):
    """vector registers named by one operand"""
    tok = tok.strip().split()[0] if tok.strip() else ""
    m = re.match(r'v\[(\d+):(\d+)\]$', tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'v(\d+)$', tok)
    return {int(m.group(1))} if m else set()


def operands(l):
    t = l.strip().split(';')[0]
    op = t.split()[0]
    return op, [a for a in t[len(op):].split(',')]


def writes(l):
    """vector registers a VALU instruction writes (the permlane swaps write both operands)"""
    op, a = operands(l)
    if not op.startswith('v_') or not a:
        return set()
    w = vregs(a[0])
    if 'swap' in op and len(a) > 1:
        w |= vregs(a[1])
    return w


def step_loop(lines):
    mf = [k for k, l in enumerate(lines) if 'v_mfma' in l]
    if not mf:
        return None
    last = mf[-1]
    heads = [k for k in range(last) if re.match(r'\.LBB\d+_\d+:.*Loop Header', lines[k])]
    if not heads:
        return None
    h = heads[-1]
    lab = re.escape(lines[h].split(':')[0])
    back = [k for k in range(last, len(lines)) if re.search(r's_c?branch\w*\s+' + lab + r'\b', lines[k])]
    return lines[h:back[-1] + 1] if back else None


bad_total = 0
for m in re.finditer(r'^(_Z\w+):[^\n]*\n', s, re.M):
    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0]
    if not pat.search(name):
        continue
    st = m.end(); en = s.index('s_endpgm', st)
    lines = s[st:en].splitlines()
    what = "whole function"
    if "--loop" in flags:
        loop = step_loop(lines)
        if loop is None:
            print(name, "no loop with MFMAs")
            continue
        lines, what = loop, "step loop"
    ins = [l.strip() for l in lines if is_instr(l)]
    c = Counter(l.split()[0] for l in ins)
    print(name, sum(c.values()), "(%s)" % what)
    print('   ', c.most_common(24))
    if "--loop" in flags:
        vm = [re.search(r'vmcnt\((\d+)\)', l).group(1) for l in ins if l.startswith('s_waitcnt') and 'vmcnt' in l]
        print('    v_mfma_f64 %d, v_fmac_f64_dpp %d, v_mov_*_dpp %d, v_permlane32_swap %d, v_permlane16_swap %d' % (
            sum(n for o, n in c.items() if o.startswith('v_mfma_f64')), c['v_fmac_f64_dpp'],
            sum(n for o, n in c.items() if o.startswith('v_mov_') and o.endswith('_dpp')),
            sum(n for o, n in c.items() if o.startswith('v_permlane32_swap')),
            sum(n for o, n in c.items() if o.startswith('v_permlane16_swap'))))
        print('    s_waitcnt vmcnt immediates, in program order:', ' '.join(vm))
    if "--dpp-hazards" in flags:
        n = bad = 0
        for k, l in enumerate(ins):
            op, a = operands(l)
            if not op.endswith('_dpp') or len(a) < 2:
                continue
            n += 1
            src = vregs(a[1])
            for p in ins[max(0, k - 2):k]:
                if writes(p) & src:
                    bad += 1
                    print('    HAZARD: %s   <- %s' % (l, p))
        print('    DPP instructions %d, with a vector write of their DPP source within 2 instructions: %d' % (n, bad))
        bad_total += bad
sys.exit(1 if bad_total else 0)
