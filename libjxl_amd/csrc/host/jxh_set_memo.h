// "Is this the set I planned last time?": the memo of a batched launch's description. Host only, no HIP types.
//
// A description built for a set of contexts (parameter blocks, workgroup maps, descriptor arrays on the device) stays
// valid while the set holds the same contexts in the same order, each at the generation it had, and, where the description
// holds something a generation does not cover (the plane buffer of a lender, which another context's upload may
// reallocate), while that word per context is the same too.
#ifndef JXH_SET_MEMO_H_
#define JXH_SET_MEMO_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace jxh {

// Ctx: anything with a `generation` member.
template <typename Ctx>
class SetMemo {
 public:
  // `extra`: NULL, or a word per context.
  bool Matches(const Ctx* const* ctxs, size_t n, const uintptr_t* extra = nullptr) const {
    bool same = ctxs_.size() == n && extra_.size() == (extra ? n : 0);
    for (size_t i = 0; same && i < n; i++) same = ctxs_[i] == ctxs[i] && gens_[i] == ctxs[i]->generation && (!extra || extra_[i] == extra[i]);
    return same;
  }
  void Remember(const Ctx* const* ctxs, size_t n, const uintptr_t* extra = nullptr) {
    ctxs_.assign(ctxs, ctxs + n);
    gens_.resize(n);
    for (size_t i = 0; i < n; i++) gens_[i] = ctxs[i]->generation;
    extra_.clear();
    if (extra) extra_.assign(extra, extra + n);
  }
  // No set matches until the next Remember (an empty one apart).
  void Forget() {
    ctxs_.clear();
    gens_.clear();
    extra_.clear();
  }
  // The remembered set.
  size_t size() const { return ctxs_.size(); }
  const Ctx* operator[](size_t i) const { return ctxs_[i]; }

 private:
  std::vector<const Ctx*> ctxs_;
  std::vector<uint64_t> gens_;
  std::vector<uintptr_t> extra_;
};

}  // namespace jxh

#endif  // JXH_SET_MEMO_H_
