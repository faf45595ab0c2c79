"""Who sets which tuning knob: every knob of csgn_tuning.h is set by a GPU test that compares the kernel it selects with
the oracle or the model, or is exempt for a reason written here.  csgn_tuning.h promises that results never depend on a
knob; a knob no GPU test sets is a form of a kernel that has never run in the suite.  A new knob without an entry fails,
and so does an entry whose file no longer names the knob."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# knob -> the GPU test file that sets it (others may too), or ("exempt", why)
LEDGER = {
    "mul_m": "tests/test_gpu_parity.py",
    "mul_ti": "tests/test_gpu_parity.py",
    "mul_nt": "tests/test_gpu_parity.py",
    "mul_flat": "tests/test_gpu_parity.py",
    "mul_bs": "tests/test_knob_forms_gpu.py",
    "mul_xcd": "tests/test_knob_forms_gpu.py",                  # 2: the tiled kernel's remap; 0 and 1: test_gpu_parity.py
    "mul_touch": "tests/test_gpu_parity.py",
    "mul_pf_kb": "tests/test_mul_flat_block_index.py",
    "stream_xcd": "tests/test_block_order_gpu.py",
    "ragged_c": "tests/test_ragged_order_gpu.py",
    "ragged_flat": "tests/test_gpu_parity.py",
    "ragged_pf": "tests/test_gpu_parity.py",
    "ragged_touch": "tests/test_gpu_parity.py",
    "ragged_m": "tests/test_gpu_parity.py",
    "perm_ballot": "tests/test_gpu_parity.py",
    "perm_narrow": "tests/test_gpu_parity.py",
    "perm_waves": "tests/test_gpu_parity.py",
    "perm_persist": "tests/test_gpu_parity.py",
    "dec_loop": "tests/test_decrypt_gpu.py",
    "enc_lds": "tests/test_gpu_parity.py",
    "enc_wave": "tests/test_gpu_parity.py",
    "enc_compact": "tests/test_gpu_parity.py",
    "shared_gpu": "tests/test_knob_forms_gpu.py",
    "compact_tag_bits": "tests/test_gpu_parity.py",
    "compact_nt": "tests/test_knob_forms_gpu.py",
    "compact_grid": "tests/test_knob_forms_gpu.py",
    "ragged_classes": "tests/test_gpu_parity.py",
    "ragged_coop": "tests/test_gpu_parity.py",
    "ragged_coop_span": "tests/test_gpu_parity.py",
    "ragged_coop_k": "tests/test_gpu_parity.py",
    "ragged_coop_touch": "tests/test_gpu_parity.py",
    "ragged_slice_mb": "tests/test_ragged_order_gpu.py",
    "ragged_coop_pipe": "tests/test_gpu_parity.py",
    "ragged_xcd_group": "tests/test_ragged_order_gpu.py",
    "ragged_coop_xcd_group": "tests/test_ragged_order_gpu.py",
    "compact_stagger_us": "tests/test_knob_forms_gpu.py",
    "zero_memset": ("exempt", "dev-only form that returned wrong data inside captured graphs, cause not pinned "
                              "(csgn_device.h, zero_words): not to be run by the suite"),
    "gate_fused": "tests/test_gates_gpu.py",
    "uint_fused": "tests/test_uint_gpu.py",
    "uint_plain_fused": "tests/test_uint_plain_gpu.py",
    "uint_lut_fused": "tests/test_uint_lut_gpu.py",
    "uint_read_fused": "tests/test_uint_read_gpu.py",
    "uint_addk_fused": "tests/test_uint_addk_gpu.py",
    "uint_add_where_form": "tests/test_uint_add_where_cpp.py",
    "uint_find_form": "tests/test_uint_find_gpu.py",
    "uint_find_rparts": "tests/test_uint_find_gpu.py",
    "matmul_form": "tests/test_matmul_gpu.py",
    "matmul_epart": "tests/test_matmul_gpu.py",
    "count_form": "tests/test_count_gpu.py",
    "count_cpart": "tests/test_count_gpu.py",
    "wsum_cpart": "tests/test_wsum_gpu.py",
    "uint_lt_select_form": "tests/test_uint_lt_select_gpu.py",
    "uint_pick_fused": "tests/test_uint_pick_gpu.py",
    "uint_pick_stage": "tests/test_uint_pick_gpu.py",
    "uint_write_fused": "tests/test_uint_write_gpu.py",
    "uint_pick_rows_form": "tests/test_uint_pick_rows_gpu.py",
    "uint_decrypt_form": "tests/test_uint_decrypt_cpp.py",
    "uint_decrypt_chunk": "tests/test_uint_decrypt_gpu.py",
    "uint_bitwise_form": "tests/test_uint_bitwise_gpu.py",
    "uint_arith_form": "tests/test_uint_arith_gpu.py",
    "launch_blocks": "tests/test_launch_split_gpu.py",
}
EXEMPT = {"zero_memset"}


def test_every_knob_is_set_by_a_gpu_test_or_exempt():
    from csgn_amd import capi
    names = capi.tuning_names()
    assert len(names) == len(set(names))
    missing, stale = sorted(set(names) - set(LEDGER)), sorted(set(LEDGER) - set(names))
    assert not missing, "knobs without an entry in tests/test_tuning_ledger.py: %s" % missing
    assert not stale, "entries for knobs the library does not have: %s" % stale
    exempt = {k for k, v in LEDGER.items() if isinstance(v, tuple)}
    assert exempt == EXEMPT, exempt
    for knob, entry in LEDGER.items():
        if isinstance(entry, tuple):
            kind, why = entry
            assert kind == "exempt" and len(why) > 20 and "\n" not in why, knob
            continue
        assert re.fullmatch(r"tests/test_\w+\.py", entry), (knob, entry)
        text = open(os.path.join(ROOT, entry)).read()
        assert "pytest.mark.gpu" in text, (knob, entry, "is no GPU test file")
        assert re.search(r"\b(%s|CSGN_%s)\b" % (re.escape(knob), re.escape(knob.upper())), text), \
            (knob, entry, "does not name the knob")
