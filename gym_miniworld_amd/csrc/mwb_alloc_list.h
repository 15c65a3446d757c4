// mwb_alloc_list.h - the one list of device allocations a handle owns (mwb_api.hip: dev_alloc adds to it, mwb_destroy frees
// from it and from nowhere else).  Plain C++, no HIP type: the free function is the caller's, so tests/alloc_list_host.cpp
// runs the list over malloc / free.
//
// A mark is the list's length.  A feature takes one before its first allocation and releases back to it when anything fails,
// so that a refused enable leaves the handle as it was; mwb_destroy releases to 0.  release() is for a buffer that is replaced
// during the handle's life (the texel tables, the mesh data, the pair list of mwb_copy_envs): its slot is emptied, not removed,
// so every mark taken before stays what it was.
#pragma once
#include <stddef.h>

#include <vector>

struct MwbAllocList {
    std::vector<void *> ptrs;   // in allocation order; null = released since

    size_t mark() const { return ptrs.size(); }
    void add(void *p) { ptrs.push_back(p); }
    size_t live() const {
        size_t n = 0;
        for (void *p : ptrs) n += p != nullptr;
        return n;
    }
    // frees what was added since `mark`, newest first; a mark at or beyond the end (released to already) frees nothing
    template <class Free>
    void release_to(size_t mark, Free &&free_fn) {
        while (ptrs.size() > mark) {
            if (ptrs.back()) free_fn(ptrs.back());
            ptrs.pop_back();
        }
    }
    // frees one pointer of the list; false (and nothing freed) if the list does not own it
    template <class Free>
    bool release(void *p, Free &&free_fn) {
        if (!p) return false;
        for (void *&q : ptrs)
            if (q == p) { free_fn(p); q = nullptr; return true; }
        return false;
    }
};
