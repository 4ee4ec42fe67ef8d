"""The MLA kernels' registers, LDS and scratch on the built code objects (no GPU needed).  The bounds are those DESIGN sections 29-32
record for each kernel and the occupancy each kernel's plan rests on -- 512 VGPRs per SIMD lane: two waves per SIMD fit 256 each,
three fit 168 (allocated in blocks of 8) -- not figures read off the current build."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = ("mla.hip.o", "mla_prefill.hip.o", "mla_verify.hip.o", "mla_e4m3.hip.o")
# kernel name -> (how many instantiations, LDS bytes, VGPR ceiling or None)
EXPECTED = {
    "mla_decode_kernel": (2, 79872, 256),         # fp16 and e4m3 cache: two workgroups of four waves per CU
    "mla_verify_kernel": (1, 92160, None),        # one workgroup per CU on the whole register file
    "mla_prefill_flash_kernel": (1, 43008, 168),  # three workgroups per CU
    "mla_kv_up_kernel": (1, 67584, 256),
    "mla_q_absorb_kernel": (1, 36864, None),
    "mla_kv_append_kernel": (2, None, None),      # the e4m3 form puts its 640-byte row together in LDS, the fp16 form uses none
}


def _kernels(llmie):
    llmie.build()
    spec = importlib.util.spec_from_file_location("ckr", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    ckr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ckr)
    ks = []
    for o in OBJECTS:
        ks += ckr.kernel_metadata(os.path.join(ROOT, "llm-inference-engine_amd", "csrc", "_obj", o))
    return [k for k in ks if "mla_" in k["name"]]


def test_mla_kernels_resources(llmie):
    ks = _kernels(llmie)
    assert len(ks) >= 12, [k["name"] for k in ks]
    bad = [k for k in ks if k["vgpr_spill"] or k["scratch"]]
    assert not bad, bad
    for name, (count, lds, vgpr) in EXPECTED.items():
        mine = [k for k in ks if name in k["name"]]
        assert len(mine) == count, (name, [k["name"] for k in mine])
        for k in mine:
            if lds is not None:
                assert k["lds"] == lds, k
            if vgpr is not None:
                assert k["vgpr"] <= vgpr, k
    assert sorted(k["lds"] for k in ks if "mla_kv_append_kernel" in k["name"]) == [0, 640]
