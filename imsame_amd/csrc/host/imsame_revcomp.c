/*
 * imsame_revcomp.c -- revComp IN OUT over the MI355X C-ABI: the drop-in for
 * the reference's reverseComplement.c, the second program that
 * bin/all_vs_all_metagenomes_IMSAME.sh calls (:47).
 *
 * Behaviour restated from the reference (reverseComplement.c:21-118,
 * commonFunctions.c:10-13):
 *   - exactly two paths, else the usage error (:27-28); errors are one
 *     "ERR**** <message> ****" line on stdout and exit(-1), status 255
 *   - the input is opened first, then the output (created or truncated), each
 *     with its own message (:37-41)
 *   - a successful run prints nothing
 *   - the records of IN go to OUT last first: header line kept, letters of
 *     the body reversed and complemented, one line per sequence (:56-112)
 * Not reproduced: the 1,000,000-record stack array (:19, :25) and the 2e9-byte
 * sequence buffer (:17) -- files of any size and any number of records run,
 * streamed through imsame_dev_revcomp_stream (the input is pread window by
 * window, the output written as it arrives).
 *
 * Extra options, accepted only after the two paths: -device D (HIP device,
 * default 0), -window_bytes N (the stream's window, default: the library's).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <inttypes.h>
#include <unistd.h>
#include "../../../include/imsame_dev.h"

/* terror(), commonFunctions.c:10-13 */
static void terror(const char *s) {
    printf("ERR**** %s ****\n", s);
    exit(-1);
}

static int src_pread(void *user, uint64_t offset, uint64_t n, uint8_t *dst) {
    const int fd = *(const int *)user;
    while (n) {
        const ssize_t r = pread(fd, dst, n > (1u << 30) ? (1u << 30) : (size_t)n, (off_t)offset);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return 1;                    /* an error, or the file shrank under us */
        dst += r; offset += (uint64_t)r; n -= (uint64_t)r;
    }
    return 0;
}

static int sink_write(void *user, const uint8_t *bytes, uint64_t n) {
    const int fd = *(const int *)user;
    while (n) {
        const ssize_t w = write(fd, bytes, n > (1u << 30) ? (1u << 30) : (size_t)n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return 1;
        bytes += w; n -= (uint64_t)w;
    }
    return 0;
}

int main(int argc, char **argv) {
    static const char *use = "USE: reverseComplement seqFile.IN reverseComplementarySeq.OUT";
    if (argc < 3) terror(use);
    int device = 0;
    uint64_t window = 0;
    for (int a = 3; a < argc; a += 2) {
        if (a + 1 >= argc) terror(use);
        if (!strcmp(argv[a], "-device")) device = atoi(argv[a + 1]);
        else if (!strcmp(argv[a], "-window_bytes")) window = strtoull(argv[a + 1], NULL, 10);
        else terror(use);
    }
    int fin = open(argv[1], O_RDONLY);
    const off_t len = fin < 0 ? -1 : lseek(fin, 0, SEEK_END);
    if (len < 0) terror("opening IN sequence FASTA file");
    int fout = open(argv[2], O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fout < 0) terror("opening OUT sequence Words file");

    imsame_ctx *ctx = NULL;
    if (imsame_dev_open(device, &ctx)) terror("Could not open the GPU device");
    uint64_t total = 0;
    const int rc = imsame_dev_revcomp_stream(ctx, src_pread, &fin, (uint64_t)len, window, sink_write, &fout, &total);
    imsame_dev_close(ctx);
    if (rc == IMSAME_E_IO) terror("Could not read the input file or write the output file");
    if (rc) terror(imsame_strerror(rc));
    close(fin);
    if (close(fout) != 0) terror("Could not read the input file or write the output file");
    return 0;
}
