"""CPU (no GPU): stonk_gemm_tn_bf16_group refuses bad arguments with the documented status codes before anything is launched
(a cap from the caller needs no device), the accumulating route of stonk_gemm_tn_bf16 with split_k <= 0 refuses an output
its 32-bit byte offsets cannot address, header / ctypes table / library agree on the new entry, and the grouped kernel's
object keeps the written-out K loop free of scratch."""
import ctypes
import importlib.util
import os
import re
import subprocess

from stonkgs_amd import _hip

OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(dY=4096, lda=768, X=8192, ldb=768, dW=16384, ldc=768, db=0, M=768, N=768, K=1024, alpha=1.0, k_dev=0):
    return (dY, lda, X, ldb, dW, ldc, db, M, N, K, alpha, k_dev)


def _group(members, cap=160, n=None):
    probs = _hip.tn_problems(members)
    return _hip.lib().stonk_gemm_tn_bf16_group(probs, len(members) if n is None else n, cap, 0)


def test_group_entry_refuses_bad_arguments():
    assert _hip.lib().stonk_gemm_tn_bf16_group(0, 1, 160, 0) == EINVAL
    assert _group([_problem()], n=0) == EINVAL and _group([_problem()], cap=-1) == EINVAL
    for null in ("dY", "X", "dW"):
        assert _group([_problem(), _problem(**{null: 0})]) == EINVAL, null
    assert _group([_problem()] * 5) == ESHAPE                                # more than 4 problems
    assert _group([_problem()], cap=2000) == ESHAPE
    # one work item per workgroup: 9 + 9 tiles do not fit 17 workgroups, 27 + 9 + 36 + 36 = 108 do not fit 107
    assert _group([_problem(), _problem()], cap=17) == ESHAPE
    big = [_problem(M=2304), _problem(), _problem(M=3072), _problem(N=3072, ldb=3072, ldc=3072)]
    assert _group(big, cap=107) == ESHAPE
    # per problem, what the single launch with split_k <= 0 refuses
    for kw in (dict(M=700), dict(M=384), dict(N=128, ldb=128), dict(N=640), dict(K=0), dict(lda=776), dict(ldb=800),
               dict(lda=1 << 23), dict(ldc=512), dict(ldc=700000), dict(M=699136)):   # (768 x 700 000 x 4 >= 2^31)
        assert _group([_problem(), _problem(**kw)]) == ESHAPE, kw
    for kw in (dict(lda=772), dict(dY=4100), dict(X=8200), dict(dW=16386), dict(db=16386)):
        assert _group([_problem(), _problem(**kw)]) == EALIGN, kw


def test_accumulate_route_refuses_what_32_bit_offsets_cannot_address():
    """M' * ldc * 4 >= 2^31, or a row stride below N': refused by the four-wave route (split_k <= 0); the entity decoder's
    175 104 x 768 (538 MB) passes the check - its launch is not tried here."""
    tn = _hip.lib().stonk_gemm_tn_bf16
    a = lambda M, ldc, split: tn(4096, M, 8192, 768, 16384, ldc, 0, M, 768, 1024, 1.0, split, 0, 0)
    for split in (0, -160, -1):
        assert a(699136, 768, split) == ESHAPE and a(768, 512, split) == ESHAPE, split
        assert a(175104 * 4, 768, split) == ESHAPE, split
    assert 175104 * 768 * 4 < 1 << 31 <= 699136 * 768 * 4


def test_header_ctypes_and_library_agree_on_the_group_entry():
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    assert re.search(r"^int stonk_gemm_tn_bf16_group\(const StonkTnProblem\* problems, int n, int cu_cap, void\* stream\);",
                     header, flags=re.M)
    assert "stonk_gemm_tn_bf16_group" in _hip.exported_symbols()
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "stonk_gemm_tn_bf16_group")
    assert _hip.lib().stonk_abi_version() == 5                               # an additive entry
    # the struct of the header, field by field, against the ctypes twin
    body = re.search(r"typedef struct StonkTnProblem \{(.*?)\} StonkTnProblem;", header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(const void\*|float\*|const int\*|int64_t|int|float) (.+)", decl)
            ctype, names = m.group(1), [n.strip() for n in m.group(2).split(",")]
            fields += [(n, ctype) for n in names]
    twin = {"const void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const int*": ctypes.c_void_p, "int64_t": ctypes.c_int64,
            "int": ctypes.c_int, "float": ctypes.c_float}
    assert [(n, twin[t]) for n, t in fields] == list(_hip.TnProblem._fields_)
    assert ctypes.sizeof(_hip.TnProblem) == 80


def test_grouped_kernel_keeps_scratch_out_of_the_k_loop():
    """The grouped object holds one kernel, at the accumulating kernel's register budget and no more scratch (272 bytes,
    reloaded once per work item), and none of its scratch traffic lies between the first and the last MFMA - the written-out
    K loop and nothing else holds them."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    # (objects are build products, not in the history: a no-op when __graft_entry__.build() has run)
    r = subprocess.run(["make", "-C", ROOT, "-j8"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = kr.kernel_resources(os.path.join(ROOT, "stonkgs_amd", "csrc", "gemm_tn_a4_group.o"))
    assert len(ks) == 1 and "gemm_tn_a4_group_kernel" in ks[0]["name"]
    k = ks[0]
    assert k["vgpr"] == 512 and k["scratch"] <= 272 and k.get("vgpr_spill", 0) <= 67, k
    ops = [x.split()[0] for x in k["listing"]]
    mfma = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
    scratch = [i for i, o in enumerate(ops) if o.startswith("scratch_")]
    assert len(mfma) >= 1024 and not [i for i in scratch if mfma[0] < i < mfma[-1]]
