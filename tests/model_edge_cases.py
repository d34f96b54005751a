"""Chains whose component PARAMETERS select the unit forms of the pipelined encoder (device/pipe_kernel.h, pipe_persist.h) and of
the three per-header decoders (spec_kernel.h, spec_dual_kernel.h, spec_team_kernel.h), for tests/test_emu_model_edges.py (the
emulator) and tests/test_gpu_model_edges.py (MI355X).  The kernels have one code path per component type AND parameter range --
a CM of one word, of up to 2 words, of up to 512 (in the LDS of the persistent launch), from 512 on (the 8 words of a byte
fetched together); a MIX2 with one weight in a register; an SSE below 8 bits; MIX lane groups by arity; H and M in LDS or not
by hh and hm; the lockstep decoder's two workgroup shapes -- and host/codegen.cpp repeats the same conditions.  Every chain
here records the forms it must take (FORMS: what the generated sources say) and which decoders take it; the CPU test holds the
generator to that record, so a threshold that moves fails there before a form silently drops out of what runs on the GPU.

Also the home of the two stress configs of tests/test_emu.py (aliasing table fetches, the MATCH ring's end) and their inputs."""
import numpy as np

from zpaq_amd import corpus

STRESS_HCOMP = """hcomp
  c++ *c=a b=c
  d= 0 *d=a
  d++ a=*b a>>= 1 *d=a
  d++ a=*b a<<= 1 *d=a
  d++ b-- a=*b a+=*c *d=a
  d++ hash *d=a
  d++ a=*c a>>= 6 *d=a
  d++ a=*c a>>= 2 *d=a
  d++ a=*c a>>= 3 *d=a
  d++ a=*c a<<= 1 *d=a
  halt
end
"""

PIPE_STRESS_CFG = """
comp 3 8 0 0 9
  0 icm 1
  1 isse 2 0
  2 cm 9 255
  3 cm 10 8
  4 match 8 10
  5 mix2 8 0 1 24 255
  6 mix 8 0 6 24 255
  7 sse 8 6 32 255
  8 mix2 9 7 6 16 255
""" + STRESS_HCOMP

MATCH_RING_CFG = """
comp 2 0 0 0 1
  0 match 10 9
hcomp
  b=a a=*d a<<= 8 a+=b *d=a halt
end
"""


def _walk(seed, n):
    return (np.cumsum(np.random.default_rng(seed).integers(-3, 4, n)) & 255).astype(np.uint8).tobytes()


def stress_inputs():
    """(datas, more, fit) of PIPE_STRESS_CFG, without the post-processing byte.  datas: tiny tables and contexts that move by
    little from byte to byte take every aliasing path.  more: MATCH with long matches, a history buffer (1 KiB) that wraps,
    candidates overlapping the byte being written.  fit: blocks that FIT the history buffer (MATCH then reads its history from
    the input): long and short repeats, runs of one byte from the block's start on, matches that reach back to the first bytes
    and across chunk boundaries."""
    datas = [_walk(1, 700), corpus.block("text", 600, 5).tobytes(), bytes(500), bytes([7, 7, 8, 8] * 150),
             corpus.block("lcg", 300, 9).tobytes(), bytes(range(256)) * 2]
    rep = bytes(np.random.default_rng(5).integers(0, 256, 97, dtype=np.uint8)) * 40
    more = [rep, corpus.block("text", 1500, 3).tobytes() * 3, bytes(3000), b"abcabcabd" * 400, corpus.block("records", 4000, 8).tobytes()]
    fit = [rep[:1000], bytes(1000), b"abcabcabd" * 100, corpus.block("text", 1000, 3).tobytes(), bytes([0, 0, 0, 5]) * 200,
           corpus.block("text", 300, 9).tobytes() * 3, b"\1" * 700, bytes(range(40)) * 20]
    return datas, more, fit


def match_ring_inputs():
    """Eight blocks around MATCH_RING_CFG's buffer size (512) and the 255 bytes below it: behind a candidate near the block's
    start lies the END of the ring, zero only while nothing has been written there (a zero run near the end, the bytes that
    follow the block's first bytes repeated behind it)."""
    Y, X = 0x59, 0x58

    def case(n):
        d = bytearray(np.random.default_rng(n).integers(1, 256, n, dtype=np.uint8).tobytes())
        d[1:3] = bytes([Y, X])
        d[n - 24] = X
        d[n - 23:n - 10] = bytes(13)
        d[n - 10:n - 8] = bytes([Y, X])
        return bytes(d)

    return [case(n) for n in (508, 512, 300, 258, 257, 256, 511, 400)]


# ---------------------------------------------------------------------------------------------------------------------------
# Inputs of the edge chains, as the coders take them (the post-processing byte 0 in front): at most 12 blocks of at most 1.5 KiB

def first_inputs():
    """The aliasing inputs of the stress config, an empty and a one-byte block, one block a byte longer than the MATCH buffer."""
    datas = stress_inputs()[0] + [b"", b"x", corpus.block("records", 1025, 11).tobytes()]
    return [b"\0" + d for d in datas]


def second_inputs():
    """Other seeds, other lengths, another order: coded with the same plan straight after first_inputs(), so that state a
    launch leaves behind (a table resident in LDS, a table smaller than what the clearing kernel writes at once) shows."""
    datas = [b"y", corpus.block("lcg", 777, 21).tobytes(), bytes([9] * 333), _walk(7, 1400), b"",
             corpus.block("text", 1111, 22).tobytes(), bytes([3, 3, 3, 200] * 64), corpus.block("pattern", 513, 23).tobytes(),
             bytes(range(255, -1, -1)) * 3, corpus.block("records", 64, 24).tobytes()]
    return [b"\0" + d for d in datas]


# ---------------------------------------------------------------------------------------------------------------------------
# The chains

def threshold_cfg(hh, hm, cm, mix2, mix2_mask, mix, mix_mask, sse):
    """PIPE_STRESS_CFG's nine components and program with the sizes that select forms as parameters; both MIX2s take the
    size and the mask."""
    return f"""
comp {hh} {hm} 0 0 9
  0 icm 1
  1 isse 2 0
  2 cm {cm} 255
  3 cm {max(cm - 1, 0)} 8
  4 match 8 10
  5 mix2 {mix2} 0 1 24 {mix2_mask}
  6 mix {mix} 0 6 24 {mix_mask}
  7 sse {sse} 6 32 255
  8 mix2 {mix2} 7 6 16 {mix2_mask}
""" + STRESS_HCOMP


# The lockstep decoder took this chain's one-word CM from the candidates it had fetched BEFORE the last bit's store
ONE_WORD_CFG = """
comp 2 0 0 0 2
  0 cm 0 255
  1 mix2 0 0 0 24 255
hcomp
  *d=a d++ a<<= 3 *d=a d++ a>>= 5 *d=a halt
end
"""


def wide_mix_cfg():
    """n = 42: CONST and CM (tables of 1 to 16 words) in turn, a MIX over all 40 of them (lane groups of 16: no bit lanes),
    a final MIX2 with one weight.  More than 32 components: the dual and the lockstep decoder decline."""
    lines = ["comp 6 4 0 0 42"]
    for i in range(40):
        lines.append(f"  {i} const {100 + 3 * i}" if i % 2 == 0 else f"  {i} cm {(i // 2) % 5} {255 if i % 4 == 1 else 12}")
    lines += ["  40 mix 8 0 40 24 255", "  41 mix2 0 40 39 24 0", "hcomp", "  c++ *c=a b=c d= 0"]
    for i in range(42):
        lines.append(("  hash *d=a d++", f"  a=*c a<<= {i % 7} *d=a d++", "  b-- a+=*b *d=a d++")[i % 3])
    return "\n".join(lines + ["  halt", "end", ""])


# MIX arities 1, 4 and 5: lane groups of 1, 1 and 2 weight quads; the third MIX reads the first one's output
ARITY_CFG = """
comp 4 0 0 0 9
  0 cm 4 255
  1 icm 3
  2 cm 9 8
  3 const 160
  4 match 6 8
  5 mix 8 0 1 24 255
  6 mix 8 0 4 24 255
  7 mix 9 1 5 16 255
  8 mix2 0 6 7 24 0
hcomp
  d= 0 *d=a d++ a<<= 2 *d=a d++ hash *d=a d++ d++ hash *d=a d++ a>>= 4 *d=a d++ *d=a d++ a<<= 1 *d=a d++ *d=a halt
end
"""

DEEP_ISSE = "x0,0ci1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1m"       # 18 rows: the lockstep decoder's 512-thread shape, side tables in the arena

# name -> (config text | method string, parameters that select forms)
CHAINS = {
    #                         hh  hm  cm mix2 mask mix mask sse
    "below":  (threshold_cfg(4, 8, 8, 7, 255, 7, 255, 7), dict(hh=4, hm=8, cm=(8, 7), mix2=(7, 255), mix=(7, 255, 6), sse=7)),
    "at":     (threshold_cfg(9, 9, 9, 8, 255, 8, 255, 8), dict(hh=9, hm=9, cm=(9, 8), mix2=(8, 255), mix=(8, 255, 6), sse=8)),
    "above":  (threshold_cfg(12, 10, 10, 10, 255, 9, 255, 9), dict(hh=12, hm=10, cm=(10, 9), mix2=(10, 255), mix=(9, 255, 6), sse=9)),
    "masked": (threshold_cfg(10, 3, 10, 9, 15, 9, 0, 9), dict(hh=10, hm=3, cm=(10, 9), mix2=(9, 15), mix=(9, 0, 6), sse=9)),
    "tiny":   (threshold_cfg(4, 0, 1, 1, 255, 0, 255, 0), dict(hh=4, hm=0, cm=(1, 0), mix2=(1, 255), mix=(0, 255, 6), sse=0)),
    "tiny0":  (threshold_cfg(4, 0, 0, 0, 255, 0, 0, 0), dict(hh=4, hm=0, cm=(0, 0), mix2=(0, 255), mix=(0, 0, 6), sse=0)),
    "h11":    (threshold_cfg(11, 3, 9, 8, 255, 8, 255, 8), dict(hh=11, hm=3, cm=(9, 8), mix2=(8, 255), mix=(8, 255, 6), sse=8)),
    "one_word": (ONE_WORD_CFG, dict(hh=2, hm=0, cm=(0,), mix2=(0, 255))),
    "wide_mix": (wide_mix_cfg(), dict(hh=6, hm=4, cm=(0, 1, 2, 3, 4), mix2=(0, 0), mix=(8, 255, 40))),
    "arity":  (ARITY_CFG, dict(hh=4, hm=0, cm=(4, 9), mix2=(0, 0), mix=(8, 255, 1))),
    "deep_isse": (DEEP_ISSE, dict()),
}
NAMES = list(CHAINS)


def header(z, name):
    cfg = CHAINS[name][0]
    return z.method_to_header(cfg)[0] if cfg.startswith("x") else z.assemble(cfg)[0]


# What the generated sources say about each chain (tests/test_emu_model_edges.py::forms reads them the same way): HCOMP's lanes
# and whether H / M live in LDS in the encoder; per encoder variant (0 throughput, 1 latency, 3 latency with a wavefront per SIMD)
# the light units with a lane per bit position (9 CM, 10 MIX2, 11 SSE) and MIX_BITS; PS_MIX_NH of the throughput shape; the MIX
# lane groups in weight quads; workgroup width and "small chain" of the latency shape; H in LDS in the wavefront decoders; the
# dual decoder's verdict (True or its reason); the lockstep decoder's threads per workgroup or its reason.
FORMS = {
    'below': {'lanes': 64, 'h_lds': True, 'm_lds': True,
        'bits0': (), 'mix_bits0': 0, 'bits1': (), 'mix_bits1': 0, 'bits3': (), 'mix_bits3': 0,
        'nh0': 1, 'ql': (2,), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'at': {'lanes': 32, 'h_lds': True, 'm_lds': False,
        'bits0': (11,), 'mix_bits0': 0, 'bits1': (9, 10, 11), 'mix_bits1': 1, 'bits3': (9, 10, 11), 'mix_bits3': 1,
        'nh0': 2, 'ql': (2,), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'above': {'lanes': 64, 'h_lds': False, 'm_lds': False,
        'bits0': (11,), 'mix_bits0': 0, 'bits1': (9, 10, 11), 'mix_bits1': 1, 'bits3': (9, 10, 11), 'mix_bits3': 1,
        'nh0': 1, 'ql': (2,), 'waves1': 8, 'small1': False, 'dec_h_lds': False, 'dual': True, 'team': 'H does not fit the LDS'},
    'masked': {'lanes': 16, 'h_lds': True, 'm_lds': True,
        'bits0': (11,), 'mix_bits0': 0, 'bits1': (9, 11), 'mix_bits1': 0, 'bits3': (9, 11), 'mix_bits3': 0,
        'nh0': 1, 'ql': (2,), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'tiny': {'lanes': 64, 'h_lds': True, 'm_lds': True,
        'bits0': (), 'mix_bits0': 0, 'bits1': (), 'mix_bits1': 0, 'bits3': (), 'mix_bits3': 0,
        'nh0': 1, 'ql': (2,), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'tiny0': {'lanes': 64, 'h_lds': True, 'm_lds': True,
        'bits0': (), 'mix_bits0': 0, 'bits1': (), 'mix_bits1': 0, 'bits3': (), 'mix_bits3': 0,
        'nh0': 1, 'ql': (2,), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'h11': {'lanes': 8, 'h_lds': True, 'm_lds': True,
        'bits0': (11,), 'mix_bits0': 0, 'bits1': (9, 10, 11), 'mix_bits1': 1, 'bits3': (9, 10, 11), 'mix_bits3': 1,
        'nh0': 2, 'ql': (2,), 'waves1': 8, 'small1': False, 'dec_h_lds': False, 'dual': True, 'team': 'H does not fit the LDS'},
    'one_word': {'lanes': 64, 'h_lds': True, 'm_lds': True,
        'bits0': (), 'mix_bits0': 0, 'bits1': (), 'mix_bits1': 0, 'bits3': (), 'mix_bits3': 0,
        'nh0': 1, 'ql': (), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'wide_mix': {'lanes': 64, 'h_lds': True, 'm_lds': True,
        'bits0': (), 'mix_bits0': 0, 'bits1': (), 'mix_bits1': 0, 'bits3': (), 'mix_bits3': 0,
        'nh0': 2, 'ql': (16,), 'waves1': 8, 'small1': False, 'dec_h_lds': True, 'dual': 'more than 32 components', 'team': 'more than 32 components'},
    'arity': {'lanes': 64, 'h_lds': True, 'm_lds': True,
        'bits0': (), 'mix_bits0': 0, 'bits1': (9,), 'mix_bits1': 1, 'bits3': (9,), 'mix_bits3': 1,
        'nh0': 2, 'ql': (1, 1, 2), 'waves1': 4, 'small1': True, 'dec_h_lds': True, 'dual': True, 'team': 384},
    'deep_isse': {'lanes': 32, 'h_lds': True, 'm_lds': False,
        'bits0': (), 'mix_bits0': 0, 'bits1': (), 'mix_bits1': 1, 'bits3': (), 'mix_bits3': 1,
        'nh0': 2, 'ql': (8,), 'waves1': 8, 'small1': False, 'dec_h_lds': True, 'dual': True, 'team': 512},
}

DUAL_DECLINES = ("wide_mix",)
TEAM_DECLINES = ("above", "h11", "wide_mix")
