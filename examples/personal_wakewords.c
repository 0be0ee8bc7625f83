/* personal_wakewords.c -- a wakeword bank from plain C: every stream carries its OWN wakeword, the batched form of one Rustpotter
 * per user (src/detector.rs:95-176,304-346: Rustpotter::new -> add_wakeword_from_file -> process_samples, once per user).
 *   rp_wakeword_bank_new_from_rpw(all users' .rpw files) -> rp_batch_detect_bank(streams, stream_wakeword[s] = user of stream s)
 * and then the same streams live, eight chunks per call, with the gain normaliser on: every user enrolled at their own loudness (the
 * .rpw records it), and every stream is normalised to ITS wakeword's level over its own window
 *   rp_stream_batch_new_bank -> rp_stream_batch_set_filters_bank -> rp_stream_batch_process per call (+ rp_stream_batch_levels)
 *
 *   gcc -std=c99 -Iinclude examples/personal_wakewords.c -Lrustpotter_amd -lrustpotter_hip -Wl,-rpath,$PWD/rustpotter_amd -o personal_wakewords
 *   ./personal_wakewords tests/golden/oye_casa_g.rpw tests/golden/alexa.rpw tests/golden/oye_casa_g_1.wav tests/golden/alexa.wav
 * Stream 0 is the first recording listening for the first wakeword, stream 1 the second recording listening for the second.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rustpotter_hip.h"

static unsigned char *read_file(const char *path, size_t *len) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return NULL; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *b = (unsigned char *)malloc(n > 0 ? (size_t)n : 1);
    if (b && n > 0 && fread(b, 1, (size_t)n, f) != (size_t)n) { free(b); b = NULL; }
    fclose(f);
    *len = n > 0 ? (size_t)n : 0;
    return b;
}

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s <a.rpw> <b.rpw> <a: 16 kHz mono i16 .wav> <b: 16 kHz mono i16 .wav>\n", argv[0]); return 2; }
    /* One second of silence (34 chunks of 30 ms) in front of and behind each recording, as examples/detect_wav.c feeds it: a detection is
     * reported only once half a window length has passed after its last matching window (src/detector.rs:398-430), so a stream that ends
     * right behind the utterance reports nothing.  The recording is taken in whole 30 ms chunks, as a live detector would be fed. */
    enum { N_USERS = 2, CHUNK = 480, PAD = 34 * CHUNK, MAX_DET = 4 };
    unsigned char *rpw[N_USERS], *wav[N_USERS];
    size_t rpw_len[N_USERS], wav_len[N_USERS], rec_len[N_USERS], n_samples = 0;
    for (int u = 0; u < N_USERS; ++u) {
        rpw[u] = read_file(argv[1 + u], &rpw_len[u]);
        wav[u] = read_file(argv[3 + u], &wav_len[u]);
        if (!rpw[u] || !wav[u] || wav_len[u] < 44) return 1;
        rec_len[u] = (wav_len[u] - 44) / 2 / CHUNK * CHUNK;   /* canonical 44-byte RIFF header, like the reference's tests (tests/detector.rs:372-399) */
        if (rec_len[u] + 2 * PAD > n_samples) n_samples = rec_len[u] + 2 * PAD;
    }
    int16_t *pcm = (int16_t *)calloc(N_USERS * n_samples, sizeof(int16_t));   /* [streams][n_samples], shorter recordings end in silence */
    if (!pcm) return 1;
    for (int u = 0; u < N_USERS; ++u) memcpy(pcm + (size_t)u * n_samples + PAD, wav[u] + 44, rec_len[u] * sizeof(int16_t));

    rp_ctx *ctx = NULL;
    if (rp_ctx_new(0, RP_CTX_HOST_POINTERS, &ctx) < 0) { fprintf(stderr, "rp_ctx_new: %s\n", rp_last_error()); return 1; }
    rp_wakeword_bank *bank = NULL;
    const uint8_t *bufs[N_USERS] = {rpw[0], rpw[1]};
    if (rp_wakeword_bank_new_from_rpw(ctx, N_USERS, bufs, rpw_len, &bank) < 0) { fprintf(stderr, "bank: %s\n", rp_last_error()); rp_ctx_free(ctx); return 1; }
    for (int u = 0; u < N_USERS; ++u) printf("wakeword %d: windows of %d frames\n", u, rp_wakeword_bank_max_len(bank, u));

    rp_config cfg;
    rp_config_default(&cfg);
    const int32_t stream_wakeword[N_USERS] = {0, 1};
    rp_batch_detection det[N_USERS * MAX_DET];
    int32_t n_det[N_USERS];
    if (rp_batch_detect_bank(ctx, pcm, RP_SAMPLE_I16, N_USERS, n_samples, n_samples, bank, stream_wakeword, &cfg.detector, det, n_det, MAX_DET,
                             NULL, NULL, 0) < 0) {
        fprintf(stderr, "rp_batch_detect_bank: %s\n", rp_last_error());
        rp_wakeword_bank_free(bank); rp_ctx_free(ctx);
        return 1;
    }
    for (int s = 0; s < N_USERS; ++s) {
        printf("stream %d (wakeword %d): %d detection(s)\n", s, (int)stream_wakeword[s], (int)n_det[s]);
        for (int i = 0; i < n_det[s] && i < MAX_DET; ++i) {
            const rp_batch_detection *d = &det[s * MAX_DET + i];
            printf("    frame %d window %d score %.7f avg_score %.7f counter %d\n", (int)d->frame, (int)d->window, d->score, d->avg_score, (int)d->counter);
        }
    }

    /* Live: the same two streams fed eight 30 ms chunks per call, every detector's state on the device, gain normaliser on. */
    enum { CALL_CHUNKS = 8 };
    rp_stream_batch *batch = NULL;
    cfg.filters.gain_normalizer.enabled = true;
    cfg.filters.gain_normalizer.min_gain = 0.5f;
    cfg.filters.gain_normalizer.max_gain = 2.0f;
    if (rp_stream_batch_new_bank(ctx, bank, stream_wakeword, &cfg.detector, N_USERS, CALL_CHUNKS, &batch) < 0 ||
        rp_stream_batch_set_filters_bank(batch, &cfg.filters) < 0) {
        fprintf(stderr, "live batch: %s\n", rp_last_error());
        rp_stream_batch_free(batch); rp_wakeword_bank_free(bank); rp_ctx_free(ctx);
        return 1;
    }
    for (int u = 0; u < N_USERS; ++u) printf("wakeword %d: enrolled at rms level %.4f\n", u, rp_wakeword_bank_rms_level(bank, u));
    int16_t *part = (int16_t *)malloc((size_t)N_USERS * CALL_CHUNKS * CHUNK * sizeof(int16_t));
    if (!part) {
        rp_stream_batch_free(batch); rp_wakeword_bank_free(bank); rp_ctx_free(ctx);
        free(pcm);
        return 1;
    }
    const size_t total_chunks = n_samples / CHUNK;
    for (size_t c = 0; c < total_chunks; c += CALL_CHUNKS) {
        const size_t n = total_chunks - c < CALL_CHUNKS ? total_chunks - c : CALL_CHUNKS;
        for (int u = 0; u < N_USERS; ++u) memcpy(part + (size_t)u * n * CHUNK, pcm + (size_t)u * n_samples + c * CHUNK, n * CHUNK * sizeof(int16_t));
        float gains[N_USERS * CALL_CHUNKS];
        if (rp_stream_batch_process(batch, part, RP_SAMPLE_I16, n, n * CHUNK, det, n_det, MAX_DET, NULL) < 0 ||
            rp_stream_batch_levels(batch, NULL, gains) < 0) {
            fprintf(stderr, "rp_stream_batch_process: %s\n", rp_last_error());
            rp_stream_batch_free(batch); rp_wakeword_bank_free(bank); rp_ctx_free(ctx);
            return 1;
        }
        for (int s = 0; s < N_USERS; ++s)
            for (int i = 0; i < n_det[s] && i < MAX_DET; ++i) {
                const rp_batch_detection *d = &det[s * MAX_DET + i];
                printf("live: slot %d (wakeword %d) chunk %d: score %.7f avg_score %.7f counter %d, gain of the call's last chunk %.1f\n", s,
                       (int)stream_wakeword[s], (int)d->frame / 3 + 1, d->score, d->avg_score, (int)d->counter, gains[(size_t)s * n + n - 1]);
            }
    }
    free(part);
    rp_stream_batch_free(batch);   /* the batch borrows the bank and the context */
    rp_wakeword_bank_free(bank);   /* the bank borrows the context: free it first */
    rp_ctx_free(ctx);
    free(pcm);
    for (int u = 0; u < N_USERS; ++u) { free(rpw[u]); free(wav[u]); }
    return 0;
}
