"""Dev tool: the static ledger of DESIGN 4.3 -- instruction classes summed over EVERY basic block of a kernel's first loop (the step loop
of dist_fast_kernel: head, step, accept, landing, controller, exits) in a `hipcc -O3 --offload-arch=gfx950 -S` dump, and the block that
holds the solves (the longest one) on its own.  asm_blocks.py prints the same classes block by block.
usage: asm_loop_ledger.py file.s <kernel-substring>      exit status 1 when the longest block holds a v_readlane / v_writelane"""
import collections, re, sys

txt = open(sys.argv[1]).read().split('\n')
key = sys.argv[2]
start = next(i for i, l in enumerate(txt) if l.startswith('_Z') and key in l and l.rstrip().split(':')[0].endswith('E') and ':' in l)
end = next(i for i in range(start, len(txt)) if 's_endpgm' in txt[i])
header = None
inside = False
blocks = []                                  # one Counter per basic block of the loop
for l in txt[start + 1:end + 1]:
    s = l.strip()
    if re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:)', s):
        if header is None and 'Loop Header' in s:
            header = 'Header=' + s.split(':')[0].lstrip('.L')
            inside = True
        else:
            inside = header is not None and header + ' ' in s + ' '
        if inside:
            blocks.append(collections.Counter())
        continue
    if not inside or not s or s.startswith((';', '.', '//')):
        continue
    blocks[-1][s.split()[0]] += 1


def row(c):
    def n(*names):
        return sum(v for k, v in c.items() if k.startswith(names))
    return collections.OrderedDict([
        ('VALU instructions', n('v_')),
        ('f64 FMA / MUL / ADD', n('v_fma_f64', 'v_fmac_f64', 'v_mul_f64', 'v_add_f64')),
        ('v_rcp_f64', n('v_rcp_f64')),
        ('v_cndmask_b32', n('v_cndmask_b32')),
        ('v_cmp_*', n('v_cmp')),
        ('v_max_f64 / v_min_f64', n('v_max_f64', 'v_min_f64')),
        ('plain v_mov_b32 / v_mov_b64', c['v_mov_b32_e32'] + c['v_mov_b64_e32'] + c['v_mov_b32_e64']),
        ('v_mov_b32_dpp', n('v_mov_b32_dpp')),
        ('v_or_b32 / v_or3_b32', n('v_or_b32', 'v_or3_b32')),
        ('v_readlane / v_writelane', n('v_readlane', 'v_writelane')),
        ('LDS instructions', n('ds_')),
        ('global loads / stores', n('global_load'), ), ])


loop = sum(blocks, collections.Counter())
step = max(blocks, key=lambda c: sum(c.values()))
print('loop %s: %d basic blocks' % (header, len(blocks)))
print('%-32s %8s %12s' % ('', 'loop', 'step block'))
ra, rb = row(loop), row(step)
for k in ra:
    print('%-32s %8d %12d' % (k, ra[k], rb[k]))
print('%-32s %8d %12d' % ('global stores', sum(v for k, v in loop.items() if k.startswith('global_store')), sum(v for k, v in step.items() if k.startswith('global_store'))))
print('%-32s %8d %12d' % ('s_nop', loop['s_nop'], step['s_nop']))
print('%-32s %8d %12d' % ('s_waitcnt', loop['s_waitcnt'], step['s_waitcnt']))
print('%-32s %8d %12d' % ('other SALU', sum(v for k, v in loop.items() if k.startswith('s_')) - loop['s_nop'] - loop['s_waitcnt'],
                          sum(v for k, v in step.items() if k.startswith('s_')) - step['s_nop'] - step['s_waitcnt']))
sys.exit(1 if rb['v_readlane / v_writelane'] else 0)
