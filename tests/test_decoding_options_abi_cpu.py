"""CPU: the C ABI of the decoding options (include/ccx.h: ccx_decode_options, the `opts` field appended to ccx_dec_select_desc and
ccx_dec_beam_desc, ccx_whisper_set_decode_options, ccx_whisper_logmel_ex) against its ctypes mirrors (clearconverse_amd/_lib.py): a
small host program compiled against the header prints every struct's size and the offsets of the new fields.  What needs no device is
called: the defaults, and the NULL-handle answers."""
import ctypes as C
import subprocess
from pathlib import Path

from clearconverse_amd import _lib
from clearconverse_amd.build import _hipcc

ROOT = Path(__file__).resolve().parent.parent

PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "ccx.h"
int main() {
  printf("ccx_decode_options %zu\n", sizeof(ccx_decode_options));
  printf("ccx_decode_options.suppress %zu\n", offsetof(ccx_decode_options, suppress));
  printf("ccx_decode_options.max_initial_timestamp_index %zu\n", offsetof(ccx_decode_options, max_initial_timestamp_index));
  printf("ccx_dec_select_desc %zu\n", sizeof(ccx_dec_select_desc));
  printf("ccx_dec_select_desc.stream_ids %zu\n", offsetof(ccx_dec_select_desc, stream_ids));
  printf("ccx_dec_select_desc.opts %zu\n", offsetof(ccx_dec_select_desc, opts));
  printf("ccx_dec_beam_desc %zu\n", sizeof(ccx_dec_beam_desc));
  printf("ccx_dec_beam_desc.x_elems %zu\n", offsetof(ccx_dec_beam_desc, x_elems));
  printf("ccx_dec_beam_desc.opts %zu\n", offsetof(ccx_dec_beam_desc, opts));
  printf("ccx_decode_rules %zu\n", sizeof(ccx_decode_rules));
  printf("ccx_dec_seq_state %zu\n", sizeof(ccx_dec_seq_state));
  return 0;
}
"""


def test_ctypes_mirrors_have_the_c_structs_layout(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    mirrors = {"ccx_decode_options": _lib.DecodeOptions, "ccx_dec_select_desc": _lib.DecSelectDesc, "ccx_dec_beam_desc": _lib.DecBeamDesc,
               "ccx_decode_rules": _lib.DecodeRules, "ccx_dec_seq_state": _lib.DecSeqState}
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == c[name], (name, C.sizeof(cls), c[name])
    for key, want in c.items():
        if "." in key:
            name, field = key.split(".")
            assert getattr(mirrors[name], field).offset == want, (key, getattr(mirrors[name], field).offset, want)
    # appended: the field that was last before is where a descriptor without `opts` has it
    assert _lib.DecSelectDesc.opts.offset == _lib.DecSelectDesc.stream_ids.offset + 8
    assert _lib.DecBeamDesc.opts.offset == _lib.DecBeamDesc.x_elems.offset + 8


def test_defaults_and_null_handles_need_no_device():
    lib = _lib.load()
    o = _lib.DecodeOptions(9, 9, 9, 9, None)
    lib.ccx_decode_options_default(C.byref(o))
    assert (o.without_timestamps, o.suppress_blank, o.max_initial_timestamp_index, o.n_suppress) == (0, 1, -2, 0) and not o.suppress
    lib.ccx_decode_options_default(None)                     # a NULL pointer is left alone
    assert lib.ccx_whisper_set_decode_options(None, C.byref(o)) == 1        # CCX_ERR_ARG
    assert lib.ccx_whisper_set_decode_options(None, None) == 1
    assert lib.ccx_whisper_graph_count(None, 0) == -1
    assert lib.ccx_whisper_set_prefix_len(None, 3) == 1
    assert lib.ccx_whisper_logmel_ex(None, None, 0, None, None, None, 1, None, None) == 1
    # a zeroed descriptor carries opts == NULL: what the existing kernel tests send
    assert not _lib.DecSelectDesc().opts and not _lib.DecBeamDesc().opts
