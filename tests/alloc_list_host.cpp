// Host program around gym_miniworld_amd/csrc/mwb_alloc_list.h for tests/test_alloc_list_host.py: the list over malloc / free.
// Every allocation is counted in and out, so that each case can say exactly which pointers were freed; under AddressSanitizer
// a double free, a free of a foreign pointer or a leak at exit ends the program with a non-zero status of its own.
//   alloc_list_host          runs every case, prints one "ok NAME" line per case
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "mwb_alloc_list.h"

static std::set<void *> g_live;
static int g_frees = 0;

static void *get(MwbAllocList &l, size_t bytes) {
    void *p = malloc(bytes);
    if (!p) exit(9);
    g_live.insert(p);
    l.add(p);
    return p;
}
static void put(void *p) {
    if (!g_live.erase(p)) { fprintf(stderr, "freed a pointer that is not live\n"); exit(8); }
    g_frees++;
    free(p);
}
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

int main() {
    {   // a mark, then k of n allocations, then release: exactly those k go, newest first
        for (int n = 0; n <= 6; n++)
            for (int k = 0; k <= n; k++) {
                MwbAllocList l;
                void *p[6];
                for (int i = 0; i < n - k; i++) p[i] = get(l, 16 + i);
                const size_t mark = l.mark();
                for (int i = n - k; i < n; i++) p[i] = get(l, 16 + i);
                g_frees = 0;
                l.release_to(mark, put);
                CHECK(g_frees == k && l.live() == (size_t)(n - k) && l.mark() == mark);
                for (int i = 0; i < n; i++) CHECK((g_live.count(p[i]) == 1) == (i < n - k));
                l.release_to(mark, put);   // twice: harmless
                l.release_to(mark + 3, put);   // a mark beyond the end: nothing
                CHECK(g_frees == k && l.live() == (size_t)(n - k));
                l.release_to(0, put);
                CHECK(g_live.empty() && l.mark() == 0);
            }
        printf("ok mark_release\n");
    }
    {   // one pointer out of the middle: the others stay, the marks taken before stay what they were
        MwbAllocList l;
        void *a = get(l, 8), *b = get(l, 8);
        const size_t mark = l.mark();
        void *c = get(l, 8), *d = get(l, 8);
        g_frees = 0;
        CHECK(l.release(b, put) && g_frees == 1 && !g_live.count(b) && l.live() == 3);
        CHECK(!l.release(b, put) && !l.release(nullptr, put) && g_frees == 1);   // not owned any more / never owned: nothing freed
        int foreign = 0;
        CHECK(!l.release(&foreign, put) && g_frees == 1);
        CHECK(l.release(c, put) && g_frees == 2);
        void *e = get(l, 8);   // the replacement of a released buffer
        l.release_to(mark, put);
        CHECK(g_frees == 4 && !g_live.count(d) && !g_live.count(e) && g_live.count(a) == 1 && l.live() == 1);
        l.release_to(0, put);
        CHECK(g_live.empty());
        printf("ok release_one\n");
    }
    {   // the destroy path: whatever is in the list at the end goes, released slots included; the leak check at exit agrees
        MwbAllocList l;
        void *p[8];
        for (int i = 0; i < 8; i++) p[i] = get(l, 100 * (i + 1));
        l.release(p[0], put); l.release(p[7], put); l.release(p[3], put);
        get(l, 5);
        g_frees = 0;
        l.release_to(0, put);
        CHECK(g_frees == 6 && g_live.empty() && l.live() == 0 && l.mark() == 0);
        l.release_to(0, put);
        CHECK(g_frees == 6);
        printf("ok destroy\n");
    }
    return 0;
}
