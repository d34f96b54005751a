// The host's half of fragmenting on the device: files divided into pieces, and the lists of the pieces' walks
// (device/fragment_kernel.h) stitched into the files' fragments.  Plain C++ over the structs of layout.h, so that the engine and
// the emulator's driver (tests/emu/fragment_emu_main.cpp) run the same code; `run` launches one batch of walks and brings back
// how each ended and its records.
//
// Round 0 walks every piece from its own start as if a cut lay there.  The state resets at every cut, so two walks over the same
// bytes are identical from the first cut they share: the true start of a piece is the last cut of the accepted list of the piece
// in front, and where that is not the piece's own start a fix-up walks from it until one of its cuts is in the piece's list --
// from there the list is the truth -- or until it has passed the piece's end.  The fix-ups of all open pieces run in one launch
// per round on provisional starts: the last cuts of the lists as they stand.  The host accepts pieces in order while their starts
// were the true ones; a fix-up that did not merge moves the starts behind it, and those pieces run again.  The first open piece
// of a file always has its true start, so every round finishes at least one piece per open file: data that never re-joins
// (constant bytes) degenerates to a serial walk and stays exact.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "layout.h"

namespace zpq {

struct FragPiece { uint32_t file, start, stop, rec_off, rec_cap; };
struct FragPlan {
  std::vector<FragPiece> pc;         // the pieces of all files, in order
  std::vector<size_t> first;         // file f's pieces: pc[first[f] .. first[f + 1])
  uint64_t nrec = 0;                 // records of round 0's lists; a fix-up of piece j writes to nrec + pc[j].rec_off
  bool pieces = false;               // some file has more than one piece: fix-ups may run
};

// false: the lists do not fit 32-bit record indices
inline bool frag_plan(const uint64_t* len, uint32_t n, uint64_t piece, uint32_t min_frag, FragPlan& pl) {
  pl.pc.clear();
  pl.first.assign((size_t)n + 1, 0);
  pl.nrec = 0;
  for (uint32_t f = 0; f < n; ++f) {
    pl.first[f] = pl.pc.size();
    const uint64_t np = len[f] ? (len[f] + piece - 1) / piece : 1;
    for (uint64_t k = 0; k < np; ++k) {
      const uint64_t a = k * piece, b = a + piece < len[f] ? a + piece : len[f];
      const uint64_t cap = frag_rec_cap(a, b, min_frag);
      if (pl.nrec + cap >= (1ull << 30)) return false;
      pl.pc.push_back(FragPiece{f, (uint32_t)a, (uint32_t)b, (uint32_t)pl.nrec, (uint32_t)cap});
      pl.nrec += cap;
    }
  }
  pl.first[n] = pl.pc.size();
  pl.pieces = pl.pc.size() > n;
  return true;
}

// Run: bool(const std::vector<FragJob>& jobs, std::vector<FragResult>& res, std::vector<std::vector<FragRec>>& lists) -- the jobs'
// lists ascend in the record array; false stops everything (the note is the callee's).  off[f] = file f's first byte in the
// device buffer.  fin[f] = the records of file f's fragments, the last one the fragment that ran into the end of file.
// rounds = the fix-up launches.
template <class Run>
bool frag_stitch(const FragPlan& pl, const uint64_t* off, const uint64_t* len, uint32_t n, uint64_t piece, Run&& run,
                 std::vector<std::vector<FragRec>>& fin, uint32_t& rounds, std::string& note) {
  const std::vector<FragPiece>& pc = pl.pc;
  const size_t m = pc.size();
  rounds = 0;
  fin.assign(n, std::vector<FragRec>());
  std::vector<FragJob> jb(m);
  for (size_t j = 0; j < m; ++j) {
    const FragPiece& p = pc[j];
    jb[j] = FragJob{off[p.file], (uint32_t)len[p.file], p.start, p.stop, p.rec_off, p.rec_cap, 0u, 0u};
  }
  std::vector<FragResult> r0;
  std::vector<std::vector<FragRec>> l0;
  if (!run(jb, r0, l0)) return false;
  struct Fix { bool have = false; uint32_t start = 0; FragResult r{}; std::vector<FragRec> recs; };
  std::vector<Fix> fix(m);
  std::vector<size_t> cur(n);                       // the first piece of the file that is not accepted yet ...
  std::vector<uint32_t> T(n, 0u);                   // ... and its true start
  std::vector<char> done(n, 0);
  for (uint32_t f = 0; f < n; ++f) cur[f] = pl.first[f];
  auto advance = [&](uint32_t f) {
    while (!done[f]) {
      const size_t j = cur[f];
      uint32_t st;
      if (T[f] == pc[j].start) {
        fin[f].insert(fin[f].end(), l0[j].begin(), l0[j].end());
        st = r0[j].status;
      } else if (fix[j].have && fix[j].start == T[f]) {
        fin[f].insert(fin[f].end(), fix[j].recs.begin(), fix[j].recs.end());
        st = fix[j].r.status;
        if (st == (uint32_t)kFragMerged) {          // from the common cut on, the piece's own list is the truth
          fin[f].insert(fin[f].end(), l0[j].begin() + fix[j].r.merge_at + 1, l0[j].end());
          st = r0[j].status;
        }
      } else break;
      if (st == (uint32_t)kFragEof) { done[f] = 1; break; }
      T[f] = fin[f].back().end;                     // (below the file's length: the walk ended at a cut in front of it)
      cur[f] = pl.first[f] + (size_t)(T[f] / piece);
    }
  };
  for (;;) {
    for (uint32_t f = 0; f < n; ++f) advance(f);
    std::vector<FragJob> fj;
    std::vector<size_t> who;
    for (uint32_t f = 0; f < n; ++f) {
      if (done[f]) continue;
      size_t j = cur[f];
      uint32_t t = T[f];                            // true for the first piece, provisional behind it
      for (;;) {
        const FragPiece& p = pc[j];
        uint32_t st = r0[j].status, end = l0[j].back().end;      // (as if the fix-up merges)
        if (t != p.start) {
          if (!(fix[j].have && fix[j].start == t)) {
            fix[j].have = false;
            fj.push_back(FragJob{off[f], (uint32_t)len[f], t, p.stop, (uint32_t)(pl.nrec + p.rec_off), p.rec_cap, p.rec_off, r0[j].count});
            who.push_back(j);
          } else if (fix[j].r.status != (uint32_t)kFragMerged) {
            st = fix[j].r.status;
            end = fix[j].recs.back().end;
          }
        }
        if (st == (uint32_t)kFragEof) break;
        t = end;                                    // (at or beyond the piece's end: the chain moves on)
        j = pl.first[f] + (size_t)(t / piece);
      }
    }
    if (fj.empty()) return true;
    ++rounds;
    std::vector<FragResult> rs;
    std::vector<std::vector<FragRec>> ls;
    if (!run(fj, rs, ls)) return false;
    for (size_t q = 0; q < fj.size(); ++q) {
      Fix& x = fix[who[q]];
      x.have = true;
      x.start = fj[q].start;
      x.r = rs[q];
      x.recs.swap(ls[q]);
      if (x.r.status == (uint32_t)kFragMerged && x.r.merge_at >= l0[who[q]].size()) { note = "fragment walk: a merge outside the list"; return false; }
    }
  }
}

// what `run` must refuse before anyone reads the lists: a walk without room, or without a record
inline bool frag_results_ok(const std::vector<FragJob>& jb, const std::vector<FragResult>& rs) {
  for (size_t i = 0; i < jb.size(); ++i)
    if (rs[i].status == (uint32_t)kFragFull || rs[i].count > jb[i].rec_cap || !rs[i].count) return false;
  return true;
}

}  // namespace zpq
