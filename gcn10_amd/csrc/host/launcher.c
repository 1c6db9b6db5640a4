/* launcher.c -- a run as one of the processes of an mpirun / srun launch: its rank, the launch's name, the closing
 * barrier.  No MPI library is linked; the processes share the log directory. */
#include "pipeline_internal.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

/* Rank and size of this process when it was started by an MPI launcher or
 * srun, read from the launcher's environment (Open MPI, MPICH/Hydra PMI,
 * Slurm); no MPI library is linked.  Keeps `mpirun -n N gcn10 ...` meaningful
 * across nodes: one process per node, each driving its node's GPUs. */
void gcn10_outer_from_env(int *rank, int *size)
{
    static const char *const names[][2] = { { "OMPI_COMM_WORLD_RANK", "OMPI_COMM_WORLD_SIZE" },
                                            { "PMI_RANK", "PMI_SIZE" },
                                            { "PMIX_RANK", "PMIX_SIZE" },
                                            { "SLURM_PROCID", "SLURM_NTASKS" } };

    *rank = 0;
    *size = 1;
    for (size_t i = 0; i < sizeof names / sizeof names[0]; i++) {
        const char *r = getenv(names[i][0]), *s = getenv(names[i][1]);

        if (r && s && atoi(s) > 1 && atoi(r) >= 0 && atoi(r) < atoi(s)) {
            *rank = atoi(r);
            *size = atoi(s);
            return;
        }
    }
}

/* The reference ends with MPI_Barrier and one "processed N blocks on R ranks" line from rank 0
 * (src/main.c:187-194).  The processes of an mpirun / srun launch share the log directory, not an MPI
 * library: every process leaves "<log_dir>/.done_<job>_<rank>" with its counts when its workers have
 * joined, and launcher rank 0 waits for all of them (GCN10_BARRIER_SECONDS, default 600) and logs the totals.
 * <job> tells launches apart (the launcher's job id from the environment, else the parent process id). */
void gcn10_job_tag(char job[96])
{
    static const char *const job_vars[] = { "SLURM_JOB_ID", "OMPI_MCA_ess_base_jobid", "PMIX_NAMESPACE", "PMI_JOBID",
                                            "GCN10_JOB_ID" };

    job[0] = '\0';
    for (size_t i = 0; i < sizeof job_vars / sizeof job_vars[0] && !job[0]; i++)
        if (getenv(job_vars[i]) && *getenv(job_vars[i]))
            snprintf(job, 96, "%s", getenv(job_vars[i]));
    if (!job[0])
        snprintf(job, 96, "p%ld", (long)getppid());     /* the ranks of one mpirun share their parent */
    for (char *c = job; *c; c++)
        if (!((*c >= '0' && *c <= '9') || (*c >= 'a' && *c <= 'z') || (*c >= 'A' && *c <= 'Z')))
            *c = '_';
}

void gcn10_closing_barrier(struct run *r, gcn10_log *log0)
{
    char job[96] = "", path[PATH_MAX], msg[512];
    const double limit = getenv("GCN10_BARRIER_SECONDS") ? atof(getenv("GCN10_BARRIER_SECONDS")) : 600.0;
    FILE *f;

    gcn10_job_tag(job);
    snprintf(path, sizeof path, "%s/.done_%s_%d", r->cfg.log_dir, job, r->outer_rank);
    f = fopen(path, "w");
    if (f) {
        fprintf(f, "%d %d %d\n", r->n_blocks, r->n_workers, atomic_load(&r->fatal) ? 1 : 0);
        fclose(f);
    }
    if (r->outer_rank != 0)
        return;
    {
        int blocks = 0, ranks = 0, arrived = 0, failed = 0;
        const double t0 = gcn10_now_seconds();

        for (int p = 0; p < r->outer_size; p++) {
            int b = 0, w = 0, bad = 0;
            bool got = false;

            snprintf(path, sizeof path, "%s/.done_%s_%d", r->cfg.log_dir, job, p);
            while (!got && gcn10_now_seconds() - t0 < limit) {
                f = fopen(path, "r");
                if (f) {
                    got = fscanf(f, "%d %d %d", &b, &w, &bad) == 3;
                    fclose(f);
                }
                if (!got)
                    usleep(2000);
            }
            if (got) {
                arrived++;
                blocks += b;
                ranks += w;
                failed += bad;
                unlink(path);
            }
        }
        snprintf(msg, sizeof msg, "all %d processes: processed %d blocks on %d ranks%s%s", r->outer_size, blocks, ranks,
                 arrived < r->outer_size ? " (some processes did not report in time)" : "",
                 failed ? " (a process ended with an error)" : "");
        gcn10_log_message(log0, arrived < r->outer_size || failed ? "ERROR" : "INFO", msg, true);
    }
}
