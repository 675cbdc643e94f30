"""CPU: env_parse of csrc/pk_env.hpp -- what every PK_* environment switch of the library reads for a given string -- compiled for the host
with g++ into a stand-alone program (its own main, nothing loaded into Python) and held to a table of strings.  The table was written out
by hand from the reads as they stood when each launcher parsed its own switch (one getenv lambda per switch in pk_capi.hip,
pk_inst_dist_fast12.hip, pk_inst_rand_fast.hip, pk_inst_tpr.hip, pk_inst_wide.hip, pk_inst_sens_rand.hip, pk_inst_net_ark.hip,
pk_inst_net_arkp.hip and pk_network.hip), not from the new header: which switch follows which rule, its value without a setting, and what
each rule makes of the strings that tell the rules apart."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "phoskintime_amd" / "csrc"

# Cases are separated by "--"; a case is a list of NAME=VALUE sets (none: the empty environment).  The word "defaults" prints the
# initialisers of Env instead, the word "live" sends the case's sets through env_parse_live alone over an Env of the empty environment.
MAIN = r"""
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include "pk_env.hpp"

static void print(const pk::Env& e) {
  std::printf("PK_WIDE_RAND_EXACT=%d\nPK_RAND_LEVEL6=%d\nPK_RAND_PARITY56=%d\nPK_TPR=%d\nPK_DIST_SCHED=%d\n", e.wide_rand_exact, e.rand_level6,
              e.rand_parity56, e.tpr, e.dist_sched);
  std::printf("PK_DIST_LAYOUT=%d\nPK_DIST_TRACE=%d\nPK_RAND_ROWS=%d\nPK_TPR_STAGE=%d\nPK_LEVEL_DEBUG=%d\n", (int)e.dist_layout, (int)e.dist_trace,
              (int)e.rand_one_row, (int)e.tpr_stage, e.level_debug);
  std::printf("PK_RAND_PARITY8_GRID=%d\nPK_RAND_PARITY7_TB=%d\nPK_RAND_PARITY6_TB=%d\nPK_RAND_SENS6_TB=%d\n", e.rand_parity8_grid, e.rand_parity7_tb,
              e.rand_parity6_tb, e.rand_sens6_tb);
  std::printf("PK_WIDE_RAND_DENSE=%d\nPK_WIDE_RAND_DRIFT=%d\nPK_WIDE_RAND_ROSW=%d\nPK_SENS_ROWS=%d\nPK_SENS_ROWS_MIN=%d\n", (int)e.wide_rand_dense,
              (int)e.wide_rand_drift, (int)e.wide_rand_rosw, e.sens_rows, e.sens_rows_min);
  std::printf("PK_ARK_LDS_PAD=%zu\nPK_ARK2_EXACT=%d\nPK_ARK_PAIR.enabled=%d\nPK_ARK_PAIR.mode=%d\n", e.ark_lds_pad, (int)e.ark2_exact,
              (int)e.ark_pair.enabled, e.ark_pair.mode);
  std::printf("PK_ARK_TOLFAC=%.17g\nPK_ARK_SAFETY=%.17g\nPK_ARK_GROW=%.17g\n", e.ark_tolfac, e.ark_safety, e.ark_grow);
  std::printf("PK_NET_THREADS=%d\nPK_NET_SENS_KC.cap16=%d\nPK_NET_SENS_KC.cap3=%d\n--\n", e.net_threads, pk::net_sens_kc(e, 16), pk::net_sens_kc(e, 3));
}

int main(int argc, char** argv) {
  std::map<std::string, std::string> vars;
  bool defaults = false, live = false;
  const auto lookup = [&vars](const char* name) -> const char* {
    const auto it = vars.find(name);
    return it == vars.end() ? nullptr : it->second.c_str();
  };
  for (int i = 1; i <= argc; ++i) {
    if (i == argc || !std::strcmp(argv[i], "--")) {
      pk::Env e = defaults ? pk::Env{} : live ? pk::env_parse([](const char*) -> const char* { return nullptr; }) : pk::env_parse(lookup);
      if (live) pk::env_parse_live(e, lookup);
      print(e);
      vars.clear(); defaults = live = false;
    } else if (!std::strcmp(argv[i], "defaults")) defaults = true;
    else if (!std::strcmp(argv[i], "live")) live = true;
    else {
      const char* eq = std::strchr(argv[i], '=');
      if (!eq) return 2;
      vars[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
  }
  return 0;
}
"""

# ---- the table.  None: the variable is not set.  STD holds the strings that tell the rules apart; every switch is held to all of them.
STD = (None, "", "0", "1", "2", "10", "00", "01", "-1", "abc", " 1", "1 ")
# what each rule of the old reads makes of STD, in order
ATOI = lambda unset: (unset, 0, 0, 1, 2, 10, 0, 1, -1, 0, 1, 1)                       # v ? atoi(v) : unset
UNLESS_0 = (1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1)                                      # !(v && v[0] == '0')
STARTS_1 = (0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1)                                      # v && v[0] == '1'
EQUALS_1 = (0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0)                                      # v && !strcmp(v, "1")
ATOI_IS_1 = (0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 1)                                     # v && atoi(v) == 1
ATOF = (0.0, 0.0, 0.0, 1.0, 2.0, 10.0, 0.0, 1.0, -1.0, 0.0, 1.0, 1.0)                # v ? atof(v) : 0.0
TOLFAC = (0.25, 0.25, 0.25, 1.0, 0.25, 0.25, 0.25, 1.0, 0.25, 0.25, 1.0, 1.0)        # atof, outside (0, 1]: 0.25
ATOL_SIZE = (0, 0, 0, 1, 2, 10, 0, 1, 2**64 - 1, 0, 1, 1)                            # v ? (size_t)atol(v) : 0
SCHED_NO_WORD = (256,) + (-1,) * 11                                                  # none of STD names a pacing policy: e ? dist_sched_parse(e) : 0x100
LAYOUT_NO_WORD = (0,) * 12                                                           # ... or a layout: no override
KC16 = (16, 16, 16, 1, 2, 10, 16, 1, 16, 16, 1, 1)                                   # atoi where 1 <= v < cap, else cap
KC3 = (3, 3, 3, 1, 2, 3, 3, 1, 3, 3, 1, 1)

# switch -> {printed key: (row over STD, {further string: value})}
TABLE = {
    "PK_WIDE_RAND_EXACT": {"PK_WIDE_RAND_EXACT": (ATOI(1), {"3": 3})},
    "PK_RAND_LEVEL6": {"PK_RAND_LEVEL6": (ATOI(0), {})},
    "PK_RAND_PARITY56": {"PK_RAND_PARITY56": (ATOI(-1), {})},
    "PK_TPR": {"PK_TPR": (ATOI(-1), {})},
    "PK_DIST_SCHED": {"PK_DIST_SCHED": (SCHED_NO_WORD, {
        "off": 0, "lead": 1, "lead:slot": 1, "lead:block": 4, "level": 2, "lead+level": 3, "level+lead": 3, "lead:slot+level": 3,
        "lead:block+level": 6, "level+lead:block": 6, "lead+lead:block": 5, "lead+lead:block+level": 7,
        "lead+lead": -1, "lead+lead:slot": -1, "level+level": -1, "lead:block+level+lead:block": -1,            # a repeated word, under either spelling
        "lead+": -1, "lead+level+": -1, "+lead": -1, "+": -1, "lead++level": -1,                              # a trailing, leading or doubled +
        "off+lead": -1, "lead+off": -1, "Lead": -1, " lead": -1, "lead ": -1, "lead:": -1, "leader": -1, "lea": -1, "on": -1})},
    "PK_DIST_LAYOUT": {"PK_DIST_LAYOUT": (LAYOUT_NO_WORD, {"8x4": 1, "wg256": 2, "shadow": 3, "8X4": 0, "shadow ": 0, " wg256": 0, "4x8": 0, "resident": 0})},
    "PK_DIST_TRACE": {"PK_DIST_TRACE": (EQUALS_1, {"true": 0})},
    "PK_RAND_ROWS": {"PK_RAND_ROWS": (EQUALS_1, {})},
    "PK_TPR_STAGE": {"PK_TPR_STAGE": (STARTS_1, {"1x": 1})},
    "PK_LEVEL_DEBUG": {"PK_LEVEL_DEBUG": (ATOI(0), {"3": 3})},
    "PK_RAND_PARITY8_GRID": {"PK_RAND_PARITY8_GRID": (ATOI(256), {"512": 512, "256": 256})},
    "PK_RAND_PARITY7_TB": {"PK_RAND_PARITY7_TB": (ATOI(0), {"8": 8, "16": 16, "12": 12})},
    "PK_RAND_PARITY6_TB": {"PK_RAND_PARITY6_TB": (ATOI(8), {"8": 8, "16": 16})},
    "PK_RAND_SENS6_TB": {"PK_RAND_SENS6_TB": (ATOI(8), {"8": 8, "16": 16})},
    "PK_WIDE_RAND_DENSE": {"PK_WIDE_RAND_DENSE": (UNLESS_0, {"0x": 0})},
    "PK_WIDE_RAND_DRIFT": {"PK_WIDE_RAND_DRIFT": (UNLESS_0, {})},
    "PK_WIDE_RAND_ROSW": {"PK_WIDE_RAND_ROSW": (ATOI_IS_1, {"1x": 1, "+1": 1, "11": 0})},
    "PK_SENS_ROWS": {"PK_SENS_ROWS": (ATOI(0), {"3": 3})},
    "PK_SENS_ROWS_MIN": {"PK_SENS_ROWS_MIN": (ATOI(0), {"6": 6, "12": 12})},
    "PK_ARK_LDS_PAD": {"PK_ARK_LDS_PAD": (ATOL_SIZE, {"4096": 4096, "65536": 65536})},
    "PK_ARK2_EXACT": {"PK_ARK2_EXACT": (UNLESS_0, {})},
    # read twice, by two rules: "00", "01" and "abc" are where they part
    "PK_ARK_PAIR": {"PK_ARK_PAIR.enabled": (UNLESS_0, {"3": 1}), "PK_ARK_PAIR.mode": (ATOI(3), {"3": 3})},
    "PK_ARK_TOLFAC": {"PK_ARK_TOLFAC": (TOLFAC, {"0.5": 0.5, "1.5": 0.25, "-0.1": 0.25, "1.0": 1.0, "1e-3": 1e-3, "0.25x": 0.25, "nan": 0.25, "inf": 0.25})},
    "PK_ARK_SAFETY": {"PK_ARK_SAFETY": (ATOF, {"0.9": 0.9, "1.5": 1.5, "-0.1": -0.1, "1e-1": 0.1})},
    "PK_ARK_GROW": {"PK_ARK_GROW": (ATOF, {"5": 5.0, "2.5": 2.5})},
    "PK_NET_THREADS": {"PK_NET_THREADS": (ATOI(0), {"64": 64, "128": 128, "256": 256, "100": 100})},
    # values below 1, and at and above the cap, leave the cap in force
    "PK_NET_SENS_KC": {"PK_NET_SENS_KC.cap16": (KC16, {"15": 15, "16": 16, "17": 16, "-3": 16, "3": 3, "4": 4}),
                       "PK_NET_SENS_KC.cap3": (KC3, {"15": 3, "16": 3, "17": 3, "-3": 3, "3": 3, "4": 3})},
}
LIVE = ("PK_NET_THREADS", "PK_NET_SENS_KC")


def expected(name):
    """[(string or None, {printed key: value})] for one switch."""
    keys = TABLE[name]
    strings = list(STD)
    for _, extra in keys.values():
        strings += [s for s in extra if s not in strings]
    out = []
    for s in strings:
        want = {}
        for key, (row, extra) in keys.items():
            assert s in STD or s in extra, f"{key}: the table has no value for {s!r}"
            want[key] = row[STD.index(s)] if s in STD else extra[s]
        out.append((s, want))
    return out


EMPTY = {key: row[0] for keys in TABLE.values() for key, (row, _) in keys.items()}          # what an empty environment gives


def build(d, name, *flags):
    exe = d / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(d / "main.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_env")
    (d / "main.cpp").write_text(MAIN)
    (d / "only.cpp").write_text('#include "pk_env.hpp"\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{CSRC}", str(d / "only.cpp")], check=True)      # stands alone: no HIP header
    return d


def run(exe, cases):
    """cases: lists of program arguments -> one {printed key: text} per case."""
    args = []
    for c in cases:
        args += list(c) + ["--"]
    r = subprocess.run([str(exe)] + args[:-1], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    blocks = r.stdout.split("--\n")
    assert blocks[-1] == "" and len(blocks) == len(cases) + 1
    return [dict(line.split("=", 1) for line in b.splitlines()) for b in blocks[:-1]]


def same(got, want):
    return float(got) == want if isinstance(want, float) else int(got) == want


def check_table(exe):
    plan = [((), None, EMPTY), (("defaults",), None, EMPTY)]            # (arguments, switch, expected values of that switch's keys)
    for name in TABLE:
        for s, want in expected(name):
            plan.append(((() if s is None else (f"{name}={s}",)), name, want))
            if name in LIVE:
                plan.append(((("live",) if s is None else ("live", f"{name}={s}")), name, want))
    got = run(exe, [p[0] for p in plan])
    assert set(got[0]) == set(EMPTY)
    for (args, name, want), g in zip(plan, got):
        for key, v in EMPTY.items():                                   # the switch reads as the table says, and no other switch moved
            w = want.get(key, v)
            assert same(g[key], w), f"{args}: {key} = {g[key]}, the old read gave {w}"
    # the live parser reads the live switches alone
    frozen = [f"{n}={'0' if n != 'PK_DIST_SCHED' else 'level'}" for n in TABLE if n not in LIVE]
    g = run(exe, [["live"] + frozen])[0]
    assert all(same(g[key], v) for key, v in EMPTY.items())
    # all switches at once
    every = run(exe, [[f"{n}=1" for n in TABLE]])[0]
    for n in TABLE:
        for key, (row, _) in TABLE[n].items():
            assert same(every[key], row[STD.index("1")]), key


def test_every_switch_reads_each_string_as_its_old_getenv_lambda_did(workdir):
    check_table(build(workdir, "env_table"))


def test_the_table_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(workdir):
    """The same program as a plain executable with nothing preloaded."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, f"-I{CSRC}", "-c", str(workdir / "main.cpp"), "-o", str(workdir / "main_san.o")],
                   check=True)
    link = subprocess.run(["g++", *san, str(workdir / "main_san.o"), "-o", str(workdir / "env_table_san")], capture_output=True, text=True)
    if link.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + link.stderr.strip().splitlines()[-1])
    check_table(workdir / "env_table_san")


def strip_comments(text):
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def test_getenv_lives_in_one_unit_and_every_switch_is_listed_once():
    for f in sorted(CSRC.iterdir()):
        if f.name != "pk_env.hip":
            assert not re.search(r"\bgetenv\b", strip_comments(f.read_text())), f"{f.name} reads the environment itself"
    assert len(re.findall(r"\bgetenv\b", strip_comments((CSRC / "pk_env.hip").read_text()))) == 2          # the snapshot and the live reader
    hdr = (CSRC / "pk_env.hpp").read_text()
    looked_up = re.findall(r'lookup\("(PK_[A-Z0-9_]+)"\)', strip_comments(hdr))
    assert sorted(looked_up) == sorted(TABLE) and len(TABLE) == 27                                            # each once; the live two in env_parse_live
    fields = re.search(r"\nstruct Env \{\n(.*?)\n\};\n", hdr, flags=re.S).group(1)
    comments = "\n".join(re.findall(r"//[^\n]*", fields))
    for name in TABLE:
        assert len(re.findall(rf"\b{name}\b", comments)) == 1, f"{name} is named in {len(re.findall(name, comments))} field comments"
    assert sorted(n for n in LIVE) == sorted(re.findall(r"\b(PK_[A-Z0-9_]+), [^.\n]*, LIVE\.", comments))
    assert len(re.findall(r", frozen\.", comments)) == len(TABLE) - len(LIVE)
