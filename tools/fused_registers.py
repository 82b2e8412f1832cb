"""Register, spill and scratch metadata of the fused posterior kernels in two built libraries, side by side:
    python tools/fused_registers.py PARENT_LIB.so NEW_LIB.so
Reads the gfx950 code object out of each library (llvm-objcopy, clang-offload-bundler, llvm-readelf --notes).  A kernel of
the first library without the trailing TAIL template argument stands beside the TAIL = false instantiation of the second."""
import subprocess, sys, re, os, tempfile
L='/opt/rocm/llvm/bin/'
def meta(lib):
    d=tempfile.mkdtemp()
    fat=os.path.join(d,'fat.bin'); co=os.path.join(d,'dev.co')
    subprocess.check_call([L+'llvm-objcopy','--dump-section','.hip_fatbin='+fat,lib,os.path.join(d,'x')])
    subprocess.check_call([L+'clang-offload-bundler','--type=o','--targets=hipv4-amdgcn-amd-amdhsa--gfx950','--input='+fat,'--output='+co,'--unbundle'])
    txt=subprocess.run([L+'llvm-readelf','--notes',co],capture_output=True,text=True).stdout
    out={}
    for blk in txt.split('  - .agpr_count:')[1:]:
        g=lambda k: (re.search(r'\.'+k+r':\s+(\S+)',blk) or [None,None])[1]
        name=g('name')
        if not name or 'k_fused_' not in name or 'rowindex' in name: continue
        dn=subprocess.run(['c++filt',name],capture_output=True,text=True).stdout.strip().split('(')[0].replace('void tehmm::','')
        out[dn]=(int(g('vgpr_count')),int(g('sgpr_count')),int(g('vgpr_spill_count')),int(g('sgpr_spill_count')),int(g('private_segment_fixed_size')))
    return out
if __name__=='__main__':
    a=meta(sys.argv[1]); b=meta(sys.argv[2])
    def key(n):
        m=re.match(r'k_fused_(\w+)<(\d+), (.*)>',n); return (m.group(1),[x.strip() for x in m.group(3).split(',')][0],int(m.group(2)),m.group(3))
    print('%-46s %-22s %s'%('kernel','parent','this commit'))
    print('%-46s %-22s %s'%('','VGPR SGPR vsp ssp scr','VGPR SGPR vsp ssp scr'))
    f=lambda t: '%4d %4d %3d %3d %3d'%t if t else '   - (no such form)'
    ndiff=0
    for n in sorted(b,key=key):
        pn=re.sub(r', false>$','>',n)          # the parent's kernels have no TAIL argument
        pa=a.get(pn) if n.endswith(', false>') else None
        d=pa is not None and pa!=b[n]
        ndiff+=d
        print('%-46s %-22s %s%s'%(n,f(pa),f(b[n]),'   <- differs' if d else ''))
    missing=[k for k in a if re.sub(r'>$',', false>',k) not in b]
    print()
    print('instantiations of the parent without a TAIL = false counterpart: %d; rows that differ: %d'%(len(missing),ndiff))
