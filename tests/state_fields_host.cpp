// Host program around gym_miniworld_amd/csrc/mwb_state_fields.h for tests/test_state_fields_host.py: two MwbDev of one
// configuration (filled from mwb_resolve_task, as mwb_create fills its own) whose per-env arrays are HOST memory, and memcpy as
// the mover - mwb_get_state / mwb_set_state and everything the latter refuses, with no device.
//   state_fields_host TASK A0 A1 A2 A3 N          then one request per line on stdin:
//     table                      field NAME OFFSET ELEM_BYTES WIDTH FLAGS            the list as the header states it
//     dump                       dev NAME KIND ELEMS v ... | dev NAME KIND ELEMS hash H    every array of the SET target
//     get FIRST COUNT [all]      rc CODE | MESSAGE, then NAME v ... per field        from the GET source ("all": entity fields too)
//     set FIRST COUNT            then NAME v ... lines and "go": rc CODE | MESSAGE   check, then put, on the SET target
//   every answer ends with a line "end".
// Element i of array number a (in the order of the array list) holds a * 65536 + i in the GET source and that + 10^9 in the SET
// target (+ 0.25 in floating point, the low byte in uint8 arrays) - distinct per array, row, env and component.  ent_order and
// n_order hold lists mwb_get_state can decode: env e has B + 1 - e % 3 entries, the agent at place e % (B + 1), slot (e + k) % B
// at place k otherwise, and 200 + k in the bytes past B + 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "mwb_state_fields.h"
#include "mwb_task_table.h"

static int mv(void *dst, const void *src, size_t bytes, bool) {
    if (bytes) memcpy(dst, src, bytes);
    return 0;
}

static const char *kind(const double *) { return "f8"; }
static const char *kind(const float *) { return "f4"; }
static const char *kind(const int32_t *) { return "i4"; }
static const char *kind(const uint32_t *) { return "u4"; }
static const char *kind(const int64_t *) { return "i8"; }
static const char *kind(const uint8_t *) { return "u1"; }
static void show(double v) { printf(" %.17g", v); }
static void show(float v) { printf(" %.9g", (double)v); }
static void show(int32_t v) { printf(" %d", v); }
static void show(uint32_t v) { printf(" %u", v); }
static void show(int64_t v) { printf(" %lld", (long long)v); }
static void show(uint8_t v) { printf(" %u", (unsigned)v); }
static void parse(const char *s, double *v) { *v = strtod(s, nullptr); }
static void parse(const char *s, int32_t *v) { *v = (int32_t)strtoll(s, nullptr, 10); }
static void parse(const char *s, uint32_t *v) { *v = (uint32_t)strtoull(s, nullptr, 10); }
static void parse(const char *s, int64_t *v) { *v = (int64_t)strtoll(s, nullptr, 10); }

struct Arr {
    std::string name;
    size_t n;
    void (*dump)(const void *, size_t);
    const void *b;
};
template <class T>
static void dump_as(const void *p, size_t n) {
    const T *v = (const T *)p;
    printf(" %s %zu", kind(v), n);
    if (n <= 4096) {
        for (size_t i = 0; i < n; i++) show(v[i]);
    } else {
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < n * sizeof(T); i++) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
        printf(" hash %llu", (unsigned long long)h);
    }
}

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    mwb_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.task = atoi(argv[1]);
    for (int i = 0; i < 4; i++) cfg.task_args[i] = atof(argv[2 + i]);
    MwbTaskFacts t;
    std::string err;
    if (mwb_resolve_task(cfg, &t, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 4; }
    MwbDev A, B;
    memset(&A, 0, sizeof(A));
    A.task = cfg.task; A.W = 8; A.H = 6; A.N = atoi(argv[6]);
    A.ent_task = t.ent_task; A.n_boxes = t.n_boxes; A.R_max = t.R_max; A.S_max = t.S_max; A.room_words = t.room_words; A.frame_words = t.frame_words;
    B = A;
    const size_t N = (size_t)A.N;
    const int nb = A.n_boxes;
    std::vector<Arr> arrs;
    std::vector<void *> owned;
    mwb_for_each_env_array(A, B, false, [&](auto *&pa, auto *&pb, const MwbEnvArray &a) {
        using T = std::remove_reference_t<decltype(*pa)>;
        const size_t n = mwb_env_array_elems(a, N), at = arrs.size() * 65536;
        pa = (T *)calloc(n, sizeof(T)); pb = (T *)calloc(n, sizeof(T));
        if (!pa || !pb) exit(9);
        owned.push_back(pa); owned.push_back(pb);
        for (size_t i = 0; i < n; i++) {
            if (std::is_floating_point<T>::value) { pa[i] = (T)((double)(at + i) + 0.25); pb[i] = (T)((double)(at + i) + 1e9 + 0.25); }
            else { pa[i] = (T)(at + i); pb[i] = (T)(at + i + 1000000000u); }
        }
        arrs.push_back(Arr{a.name, n, dump_as<T>, pb});
    });
    if (A.ent_task)
        for (MwbDev *d : {&A, &B})
            for (size_t e = 0; e < N; e++) {
                d->n_order[e] = nb + 1 - (int)(e % 3);
                for (int k = 0; k < MWB_ORDER_STRIDE; k++)
                    d->ent_order[e * MWB_ORDER_STRIDE + k] = (uint8_t)(k > nb ? 200 + k : k == (int)(e % (nb + 1)) ? MWB_ENT_AGENT : (e + k) % nb);
            }

    char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "table") {
            mwb_state st;
            memset(&st, 0, sizeof(st));
            mwb_for_each_state_field(st, A, [&](auto *host, auto *, const MwbStateField &f) {
                printf("field %s %zu %zu %zu %u\n", f.name, f.offset, sizeof(*host), f.width, f.flags);
            });
        } else if (cmd == "dump") {
            for (const Arr &a : arrs) { printf("dev %s", a.name.c_str()); a.dump(a.b, a.n); printf("\n"); }
        } else if (cmd == "get") {
            int first = 0, count = 0;
            std::string all;
            in >> first >> count >> all;
            mwb_state st;
            memset(&st, 0, sizeof(st));
            std::vector<std::vector<char>> bufs;
            mwb_for_each_state_field(st, A, [&](auto *&host, auto *, const MwbStateField &f) {
                if ((f.flags & MWB_SF_ENT) && !A.ent_task && all != "all") return;
                using T = std::remove_reference_t<decltype(*host)>;
                bufs.emplace_back((count * ((f.flags & MWB_SF_BOX) ? nb : 1) * f.width + 1) * sizeof(T), (char)0x5A);
                host = (T *)bufs.back().data();
            });
            std::string why;
            const int rc = mwb_state_get(A, first, count, &st, mv, &why);
            printf("rc %d | %s\n", rc, why.c_str());
            mwb_for_each_state_field(st, A, [&](auto *host, auto *, const MwbStateField &f) {
                if (!host || rc) return;
                printf("%s", f.name);
                const size_t n = count * ((f.flags & MWB_SF_BOX) ? nb : 1) * f.width;
                for (size_t i = 0; i <= n; i++) show(host[i]);   // one past the end: the 0x5A pattern still there
                printf("\n");
            });
        } else if (cmd == "set") {
            int first = 0, count = 0;
            in >> first >> count;
            mwb_state st;
            memset(&st, 0, sizeof(st));
            std::vector<std::vector<char>> bufs;
            while (fgets(line, sizeof(line), stdin)) {
                std::istringstream row(line);
                std::string name;
                row >> name;
                if (name == "go") break;
                std::vector<std::string> vals;
                for (std::string v; row >> v;) vals.push_back(v);
                bool known = false;
                mwb_for_each_state_field(st, B, [&](auto *&host, auto *, const MwbStateField &f) {
                    if (name != f.name) return;
                    using T = std::remove_reference_t<decltype(*host)>;
                    bufs.emplace_back((vals.size() + 1) * sizeof(T));
                    host = (T *)bufs.back().data();
                    for (size_t i = 0; i < vals.size(); i++) parse(vals[i].c_str(), &host[i]);
                    known = true;
                });
                if (!known) { fprintf(stderr, "no field %s\n", name.c_str()); return 6; }
            }
            std::string why;
            int rc = mwb_state_check(B, first, count, &st, mv, &why);
            if (!rc) rc = mwb_state_put(B, first, count, &st, mv);
            printf("rc %d | %s\n", rc, why.c_str());
        } else {
            return 5;
        }
        printf("end\n");
        fflush(stdout);
    }
    for (void *p : owned) free(p);
    return 0;
}
