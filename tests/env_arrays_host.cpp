// Host program around the per-env array list of gym_miniworld_amd/csrc/mwb_internal.h for tests/test_env_arrays_host.py: two
// MwbDev of one configuration (filled from mwb_resolve_task, as mwb_create fills its own) and N_SRC / N_DST envs, no device.
//   env_arrays_host TASK A0 A1 A2 A3 N_SRC N_DST WANT_DEPTH FRAME_REUSE
//     array NAME minor rows per type_size elems_src elems_dst copied     every array mwb_create would allocate, in list order
//     copy rows elem src_stride dst_stride                               every descriptor mwb_copy_envs would build
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mwb_internal.h"
#include "mwb_task_table.h"

int main(int argc, char **argv) {
    for (int n = 1; n <= MWB_MAX_ENTS; n++)
        if (mwb_task_frame_words(n) != MWB_FRAME_WORDS_FOR(n)) { fprintf(stderr, "frame words differ at %d\n", n); return 3; }
    if (argc != 10) return 2;
    mwb_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.task = atoi(argv[1]);
    for (int i = 0; i < 4; i++) cfg.task_args[i] = atof(argv[2 + i]);
    MwbTaskFacts t;
    std::string err;
    if (mwb_resolve_task(cfg, &t, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 4; }
    MwbDev s, d;
    memset(&s, 0, sizeof(s));
    s.task = cfg.task; s.W = 80; s.H = 60; s.want_depth = atoi(argv[8]);
    s.ent_task = t.ent_task; s.n_boxes = t.n_boxes; s.R_max = t.R_max; s.S_max = t.S_max; s.room_words = t.room_words; s.frame_words = t.frame_words;
    d = s;
    s.N = atoi(argv[6]); d.N = atoi(argv[7]);
    mwb_for_each_env_array(s, d, atoi(argv[9]) != 0, [&](auto *&sp, auto *&, const MwbEnvArray &a) {
        printf("array %s %d %u %zu %zu %zu %zu %d\n", a.name, a.minor ? 1 : 0, a.rows, a.per, sizeof(*sp), mwb_env_array_elems(a, (size_t)s.N),
               mwb_env_array_elems(a, (size_t)d.N), a.not_copied ? 0 : 1);
        if (a.not_copied && !a.not_copied[0]) exit(5);   // an array left out of the copy says why
    });
    mwb_for_each_copied_array(s, d, [&](const char *, char *, uint32_t rows, uint32_t elem, uint64_t ss, uint64_t ds) {
        printf("copy %u %u %llu %llu\n", rows, elem, (unsigned long long)ss, (unsigned long long)ds);
    });
    return 0;
}
