#!/usr/bin/env python3
"""Per-kernel digests of two builds of a library's device code, side by side (no GPU needed):

    python3 tools/isa_compare.py PARENT_LIB NOW_LIB [REPO]

Every kernel of both fat binaries is disassembled as tools/dump_isa.sh does it (llvm-objdump -d --no-show-raw-insn of the unbundled
gfx950 code object); per kernel the sha256 (16 hex digits) of the text from its symbol line to its last instruction, with the
address in front of every line, everything behind the // of the trailing comment and the names of branch targets stripped and the
padding behind the last instruction dropped.  Prints the kernels that are unchanged, differing, gone and new, then the resources
(tools/kernel_resources.sh) of the exact-search kernels of NOW_LIB.  PARENT_LIB is the parent commit's build, made in a
`git worktree` of it by its own build_library.  profiles/learner/exact_limited_isa.log is its output."""
import hashlib, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    tmp = tempfile.mkdtemp()
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section", f".hip_fatbin={fat}", lib], check=True)
    blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    out = {}
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(blob)
        b = os.path.join(tmp, f"b{n}.bin")
        open(b, "wb").write(blob[s:e])
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={b}",
                        f"--output={b}.co", "--unbundle"], stderr=subprocess.DEVNULL)
        if not os.path.exists(b + ".co") or os.path.getsize(b + ".co") == 0:
            continue
        txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", b + ".co"], capture_output=True, text=True).stdout
        name, lines = None, []
        for line in txt.splitlines() + ["0 <end>:"]:
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                if name and "kernel" in name:
                    body = [re.sub(r"^\s*[0-9a-f]+:", "", re.sub(r"//.*$", "", x)).rstrip() for x in lines]
                    while body and (not body[-1].strip() or "s_nop" in body[-1] or "s_code_end" in body[-1]):
                        body.pop()
                    body = [re.sub(r"<[^>]*>", "<>", x) for x in body]
                    out[name] = (hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body),
                                 sum(1 for x in body if x.strip().startswith("v_")))
                name, lines = m.group(1), []
            elif name:
                lines.append(line)
    return out


def resources(lib, repo):
    txt = subprocess.run(["bash", os.path.join(repo, "tools/kernel_resources.sh"), lib], capture_output=True, text=True).stdout
    res = {}
    for line in txt.splitlines():
        p = line.split()
        if len(p) >= 9:
            res[p[8]] = line.rstrip()
    return res, txt


parent, now = sys.argv[1:3]
repo = sys.argv[3] if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = kernels(parent), kernels(now)
same = [k for k in A if k in B and A[k][0] == B[k][0]]
diff = [k for k in A if k in B and A[k][0] != B[k][0]]
gone = [k for k in A if k not in B]
new = [k for k in B if k not in A]
print(f"# 1. unchanged, instruction for instruction: {len(same)} of the parent's {len(A)} kernels")
for k in sorted(same, key=lambda k: (len(k), k)):
    print(f"{k}: {A[k][0]} parent, {B[k][0]} now, {A[k][1]} lines")
print(f"# 2. differing: {len(diff)}")
for k in diff:
    print(f"{k}: {A[k][0]} parent, {B[k][0]} now; lines {A[k][1]} -> {B[k][1]}; v_ lines {A[k][2]} -> {B[k][2]}")
print(f"# 3. gone: {len(gone)}")
for k in gone:
    print(k)
print(f"# 4. new: {len(new)}")
rb, txt = resources(now, repo)
for k in sorted(new, key=lambda k: (len(k), k)):
    print(f"{k}: {B[k][0]} now, {B[k][1]} lines, {B[k][2]} v_ lines")
print("# kernel resources of the new kernels and of their twins (tools/kernel_resources.sh): VGPRs, SGPRs, scratch and static LDS bytes")
for line in txt.splitlines():
    if re.search(r"exact|window", line) and "nodes" not in line and "labels" not in line:
        print(line.rstrip())
tot = sum(int(l.split()[4]) for l in txt.splitlines() if len(l.split()) >= 9 and l.split()[4].isdigit())
print(f"# scratch bytes summed over every kernel of the library: {tot}")
