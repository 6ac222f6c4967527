"""Per-kernel digest of the gfx950 code hipcc generates for csrc/*.hip, to check on a machine without a GPU that a source change
left the device code alone.

    python tools/isa_digest.py --out after.json [--csrc DIR] [--text-dir DIR]
    python tools/isa_digest.py --compare before.json after.json [--table SUBSTR ...]

Every .hip file is compiled to assembly with the product flags of _build.py (both builds of the files built twice).  Per kernel
(mangled name -- the file a kernel lives in is not part of the key, so a kernel may move between files): a hash of its instruction
text with comments, directives and the per-file numbering of local labels dropped, the register / LDS / scratch figures of its
kernel descriptor, and the counts of the instruction classes the conv kernels are built around.  --csrc digests another tree's
sources (a checkout of the commit to compare against) with this tree's flags; --text-dir keeps the normalised text per kernel
for `diff`.  --compare prints every kernel whose digest differs and returns 1 if any does; --table prints the figures of the
kernels whose name contains one of the substrings, first file beside second."""
import argparse
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'boosting-neural-video-representation-via-online-structural-reparameteration_amd')
COUNTED = ('v_mfma', 'ds_read_b128', 'ds_read_b64_tr_b16', 'global_load_lds', 's_barrier', 's_waitcnt', 'buffer_store', 'global_store')
FIGURES = ('next_free_vgpr', 'num_agpr', 'next_free_sgpr', 'group_segment_fixed_size', 'private_segment_fixed_size', 'occupancy')


def _build_module():
    spec = importlib.util.spec_from_file_location('orn_build', os.path.join(PKG, '_build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _assemble(b, src, extra, out):
    cmd = [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(os.path.basename(src), []) + extra + ['--cuda-device-only', '-S', src, '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed for {src}:\n{r.stderr}')
    with open(out) as f:
        return f.read()


# local labels carry the index of their function within the file (.LBB3_7, .Lfunc_end3): dropped, so that a kernel keeps its text
# when a neighbour moves out of the file
_LABEL = re.compile(r'\.L([A-Za-z_]+?)\d+(_\d+)?\b')


def digest_asm(text):
    """{mangled kernel name: digest} of one assembly file"""
    out = {}
    name, body = None, []
    funcs = {}
    for line in text.splitlines():
        m = re.match(r'^([A-Za-z_$][\w$.]*):', line)
        if m and not line.startswith('.L'):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith('.Lfunc_end'):
            funcs[name] = body
            name = None
            continue
        code = line.split(';', 1)[0].rstrip()
        if not code.strip():
            continue
        if code.strip().startswith('.') and not code.rstrip().endswith(':'):      # directives (.file, .ident, .section, the .amdhsa_ block ...)
            continue
        body.append(_LABEL.sub(lambda k: '.L' + k.group(1) + (k.group(2) or ''), code).strip())
    for kern in re.findall(r'^\t\.amdhsa_kernel (\S+)$', text, re.M):
        desc = text.split(f'\t.amdhsa_kernel {kern}\n', 1)[1]
        info = desc.split('; Kernel info:', 1)[1].split('.section', 1)[0]
        desc = desc.split('.end_amdhsa_kernel', 1)[0]

        def field(key, where=desc, pat=r'\.amdhsa_%s (\d+)'):
            return int(re.search(pat % key, where).group(1))
        instr = funcs[kern]
        d = {'sha256': hashlib.sha256('\n'.join(instr).encode()).hexdigest(), 'n_lines': len(instr),
             'next_free_vgpr': field('next_free_vgpr'), 'num_agpr': field('NumAgprs', info, r'; %s: (\d+)'),
             'next_free_sgpr': field('next_free_sgpr'), 'group_segment_fixed_size': field('group_segment_fixed_size'),
             'private_segment_fixed_size': field('private_segment_fixed_size'), 'occupancy': field('Occupancy', info, r'; %s: (\d+)')}
        for c in COUNTED:
            d[c] = sum(1 for i in instr if i.startswith(c))
        d['text'] = instr
        out[kern] = d
    return out


def digest_tree(csrc, text_dir=None):
    b = _build_module()
    jobs = [(os.path.join(csrc, f), suffix, extra) for f in sorted(os.listdir(csrc)) if f.endswith('.hip') for suffix, extra in b.variants(f)]
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        def run(job):
            src, suffix, extra = job
            return digest_asm(_assemble(b, src, extra, os.path.join(tmp, os.path.basename(src)[:-4] + suffix + '.s')))
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            for job, kernels in zip(jobs, ex.map(run, jobs)):
                for k, d in kernels.items():
                    assert k not in result, f'{k} is defined twice'
                    text = d.pop('text')
                    if text_dir:
                        os.makedirs(text_dir, exist_ok=True)
                        with open(os.path.join(text_dir, k[:200] + '.s'), 'w') as f:
                            f.write('\n'.join(text) + '\n')
                    result[k] = d
    return result


def compare(a, b, table):
    differ = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f'{"only in second" if k not in a else "only in first"}: {k}')
            differ += 1
        elif a[k] != b[k]:
            keys = [f for f in a[k] if a[k][f] != b[k].get(f)]
            print(f'differs ({", ".join(keys)}): {k}')
            differ += 1
    print(f'{len(a)} / {len(b)} kernels, {differ} differ')
    cols = FIGURES + COUNTED + ('n_lines',)
    for k in sorted(set(a) & set(b)):
        if any(s in k for s in table):
            print(k)
            for c in cols:
                print(f'    {c:28s} {a[k][c]:6d} {b[k][c]:6d}' + ('' if a[k][c] == b[k][c] else '   <--'))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', help='write the digest of the tree as JSON')
    ap.add_argument('--csrc', default=os.path.join(PKG, 'csrc'), help='source directory to digest (default: this tree)')
    ap.add_argument('--text-dir', help='also keep the normalised instruction text, one file per kernel')
    ap.add_argument('--compare', nargs=2, metavar=('FIRST', 'SECOND'))
    ap.add_argument('--table', nargs='*', default=[], help='with --compare: print the figures of kernels whose name contains one of these')
    args = ap.parse_args()
    if args.compare:
        with open(args.compare[0]) as f, open(args.compare[1]) as g:
            return compare(json.load(f), json.load(g), args.table)
    if not args.out:
        ap.error('--out or --compare')
    d = digest_tree(args.csrc, args.text_dir)
    with open(args.out, 'w') as f:
        json.dump(d, f, indent=1, sort_keys=True)
    print(f'{len(d)} kernels -> {args.out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
