#!/bin/bash
# Instruction counts per step-loop region of a kernel (tools only): builds the
# library variant `marks` with -DRHMC_MARKS (s_setprio markers in
# rhmc_k1step.hpp; `make variant`, both translation units) and splits the
# disassembly at the markers.  usage: [EXTRA=-D...] isa_regions.sh NAME_SUBSTRING
ROOT=$(cd "$(dirname "$0")/.." && pwd)
make -s -C "$ROOT/hmc-stellar-toy-model_amd" variant NAME=marks FLAGS="-DRHMC_MARKS ${EXTRA:-}" || exit 1
mkdir -p /tmp/isa; cd /tmp/isa || exit 1
/opt/rocm/lib/llvm/bin/llvm-objcopy --dump-section=.hip_fatbin=fatm.bin "$ROOT/build/variants/lib_marks.so"
python3 - "$1" <<'PY'
import re,subprocess,sys
from collections import Counter
LLVM='/opt/rocm/lib/llvm/bin/'
# one offload bundle per translation unit, concatenated by the linker
data=open('fatm.bin','rb').read()
starts=[m.start() for m in re.finditer(rb'__CLANG_OFFLOAD_BUNDLE__',data)]
funcs={};cur=None
for i,st in enumerate(starts):
    open('b%d.bin'%i,'wb').write(data[st:starts[i+1] if i+1<len(starts) else len(data)])
    subprocess.run([LLVM+'clang-offload-bundler','--unbundle','--type=o','--input=b%d.bin'%i,
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950','--output=km%d.co'%i],check=True)
    out=subprocess.run([LLVM+'llvm-objdump','-d','--mcpu=gfx950','km%d.co'%i],check=True,
                       capture_output=True,text=True).stdout
    for line in out.splitlines():
        m=re.match(r"^[0-9a-f]+ <(\S+)>:",line)
        if m: cur=m.group(1); funcs[cur]=[]; continue
        if cur and line.strip(): funcs[cur].append(line.split('//')[0].strip())
k=[k for k in funcs if sys.argv[1] in k][0]
v=funcs[k]
open('m.s','w').write('\n'.join(v))
seg='start'; counts={}
for l in v:
    op=l.split()[0] if l else ''
    if op=='s_setprio':
        seg=l; counts.setdefault(seg,Counter()); continue
    c=counts.setdefault(seg,Counter())
    for p,n in (('v_','valu'),('s_','salu'),('ds_','lds')):
        if op.startswith(p): c[n]+=1
    if op.startswith('s_cbranch') or op.startswith('s_branch'): c['br']+=1
for s,c in counts.items(): print(s, dict(c))
PY
