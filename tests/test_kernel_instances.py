"""The table of world-kernel instances (kernel_instances.py) is complete: the mangled kernel names are plain strings in the built library, so
the set of compiled instances of the seven world-kernel families is read from the library's bytes (names only — nothing is disassembled) and
must equal the set the table names, in both directions.  A new instantiation without a row fails here, and so does a row for an instance that
no longer exists."""
import os
import re

import kernel_instances as KI
from test_quad_select_paths import CONFIGS

_MANGLED = re.compile(rb"_Z(\d+)(hh_k_[A-Za-z0-9_]+)")
_TEMPLATE_ARGS = re.compile(rb"I((?:L[ib]\d+E)+)E")
_ARG = re.compile(rb"L([ib])(\d+)E")


def compiled_kernels(blob):
    """{kernel name: set of template-argument strings ("" for a kernel that is no template)} of every _Z<len>hh_k_... in `blob`"""
    out = {}
    for m in _MANGLED.finditer(blob):
        n = int(m.group(1))
        name = m.group(2)
        if len(name) < n:
            continue                       # the length prefix runs past the identifier: not a name of ours
        name, rest = name[:n], blob[m.start(2) + n:m.start(2) + n + 256]
        if not name.startswith(b"hh_k_"):
            continue
        t = _TEMPLATE_ARGS.match(rest)
        args = ""
        if t:
            args = ", ".join(("true" if v != b"0" else "false") if k == b"b" else v.decode() for k, v in _ARG.findall(t.group(1)))
        out.setdefault(name.decode(), set()).add(args)
    return out


def _library_bytes():
    from hhmarl_2d_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), f"{_lib.LIB_PATH} is not built"
    with open(_lib.LIB_PATH, "rb") as f:
        return f.read()


def test_mangled_name_parser():
    blob = (b"\0_Z15hh_k_world_quadILi1ELi0ELb1ELi8ELb0ELb1EEv7DevPtrs6DevCfgiPKaPfS4_PhS5_\0_Z15hh_k_world_quadILi1ELi0ELb1ELi8ELb0ELb1EEv7DevPtrs.kd\0"
            b"_Z10hh_k_worldILi4ELi64ELi2ELb0EEv7DevPtrs\0_Z15hh_k_pack_statsiPKfPKiPKaPf\0_Z30__device_stub__hh_k_pack_statsiPKf\0")
    assert compiled_kernels(blob) == {"hh_k_world_quad": {"1, 0, true, 8, false, true"}, "hh_k_world": {"4, 64, 2, false"}, "hh_k_pack_stats": {""}}


def test_table_names_exactly_the_compiled_instances():
    got = compiled_kernels(_library_bytes())
    print(len(got), "distinct hh_k_* kernels,", sum(len(v) for v in got.values()), "instances")
    compiled = {f"{fam}<{args}>" for fam in KI.FAMILIES for args in got.get(fam, ())}
    for fam in KI.FAMILIES:
        assert got.get(fam), f"no instance of {fam} in the library"
        print(fam, len(got[fam]))
    table = KI.table_instances()
    assert {KI.family(i) for i in table} <= set(KI.FAMILIES)
    assert not compiled - table, f"compiled instances without a row in kernel_instances.py: {sorted(compiled - table)}"
    assert not table - compiled, f"rows of kernel_instances.py for instances the library does not hold: {sorted(table - compiled)}"


def test_rows_are_well_formed():
    for r in KI.ROWS:
        assert set(r["env"]) <= set(KI.SWITCHES) and r["instances"] and r["sizes"], r
        assert r["path"] in ("rollout", "split-step", "phases", "hl_rollout", "variant-rows"), r
        fams = {KI.family(i) for i in r["instances"]}
        assert len(fams) == 1, r
        if r["printed"] is not None:       # the printed name is the row's instance, or stands for its phases
            assert KI.family(r["printed"]) in fams, r
            assert r["printed"] in r["instances"] or r["printed"].endswith(", phase>"), r
        if r in KI.QUAD_ROWS:
            assert r["config"] in CONFIGS or r["config"] == "l4-split", r
        else:
            assert r["config"] in KI.HL_CONFIGS, r
    assert sum(len(paths) for _, _, paths in KI.hl_settings()) == len(KI.HIER_ROWS)


def test_rows_cover_what_the_forms_must_run():
    """every preset, and PRE = 0 with both general configurations, in each of the five 2-vs-2 forms; "l3-stay-done" on every PRE = 1 instance"""
    forms = [dict(HH_NO_TWO="1"), dict(HH_FORCE_W="2"), dict(), dict(HH_NO_DUAL="1"), dict(HH_APW="16")]
    for env in forms:
        cfgs = {r["config"] for r in KI.QUAD_ROWS if r["env"] == env and r["path"] == "rollout"}
        assert set(KI.PRESET) <= cfgs, (env, set(KI.PRESET) - cfgs)
    pre1 = {r["instances"][0] for r in KI.QUAD_ROWS if r["instances"][0].startswith("hh_k_world_quad<") and r["instances"][0].split(", ")[1] == "1"}
    stay = {r["instances"][0] for r in KI.QUAD_ROWS if r["config"] == "l3-stay-done"}
    assert pre1 and pre1 == stay
