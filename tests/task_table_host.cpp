// Host program around gym_miniworld_amd/csrc/mwb_task_table.h for tests/test_task_table_host.py (no HIP: a plain C++ compiler).
//   task_table_host rows                              one line per row: task name n_meshes geometry...
//   task_table_host resolve TASK A0 A1 A2 A3 STEPS    mwb_resolve_task on that config: "rc | facts..." or "rc | message"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mwb_task_table.h"

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "rows")) {
        for (const MwbTaskRow &r : MWB_TASK_TABLE) {
            printf("%d %s %d", r.task, r.name, r.n_meshes);
            for (int k = 0; k < r.n_meshes; k++) printf(" %d", r.meshes[k]);
            printf("\n");
        }
        return 0;
    }
    if (argc != 8 || strcmp(argv[1], "resolve")) return 2;
    mwb_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = MWB_ABI_VERSION;
    cfg.task = atoi(argv[2]);
    for (int i = 0; i < 4; i++) cfg.task_args[i] = atof(argv[3 + i]);
    cfg.max_episode_steps = atoi(argv[7]);
    MwbTaskFacts t;
    std::string err;
    const int rc = mwb_resolve_task(cfg, &t, &err);
    if (rc) { printf("%d | %s\n", rc, err.c_str()); return 0; }
    printf("%d | %d %d %d %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g\n", rc, t.n_boxes, t.R_max, t.S_max, t.max_episode_steps, t.n_tex,
           t.no_ceiling, t.poly, t.room_words, t.frame_words, t.ent_task, t.agent_radius, t.task_args[0], t.task_args[1], t.task_args[2],
           t.task_args[3]);
    return 0;
}
