// TEST INFRASTRUCTURE -- the checker of xrt_compose_hits and xrt_fold_samples: the return path of RayTracer.CastRay (RT:584, 699, 705, 726, 732)
// and the supersampling fold (RT:309) of the CPU oracle, on caller-given terms.  The oracle is included unmodified (through the checker of
// xrt_cast_rays, whose orc_cast_rays this library exports too); its CastRay keeps these statements between its nested calls, so this
// translation unit restates them with "the nested call returned reflect_rgba[i] / refract_rgba[i]" in the calls' place, written with the
// oracle's own Lerp, ColorFromVector3 (`new Color(Vector3)`) and ColorToVector3 (`ToVector3()`).
// tests/test_compose_cpu.py pins the restatement against the oracle's CastRay and against its XRT_MS_FIXED16 frames.
#include "../castray/castray_ref.cpp"

extern "C" {

// for every i: the colour vector and the colour of include/xrt.h xrt_compose_hits.  Either output may be null.
// counts_out (nullable, 4 words): [0] entries with XRT_SURF_HIT   [1] entries that took RT:699   [2] vectors with a NaN   [3] entries without XRT_SURF_HIT
int orc_compose_hits(const xrt_surface *surface, const float *light, const uint32_t *reflect_rgba, const uint32_t *refract_rgba, int64_t n,
                     uint32_t *rgba_out, float *rgb_f32_out, uint64_t *counts_out) {
    if (refract_rgba && !reflect_rgba) return -2;
    uint64_t counts[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) {
        const xrt_surface &s = surface[i];
        Vector3 colorVector = V3(0, 0, 0);   // RT:732
        if (s.flags & XRT_SURF_HIT) {
            counts[0]++;
            const Vector3 surfaceColor = V3(s.color[0], s.color[1], s.color[2]);
            const Vector3 lightResult = V3(light[3 * i], light[3 * i + 1], light[3 * i + 2]);
            if (!reflect_rgba) {
                colorVector = lightResult * surfaceColor;   // RT:726
            } else {
                colorVector = Lerp(ColorToVector3(reflect_rgba[i]), surfaceColor, 1.0f - s.reflectiveness) * lightResult;   // RT:584
                if (refract_rgba && (s.flags & XRT_SURF_TRANSPARENT)) {
                    colorVector = Lerp(ColorToVector3(refract_rgba[i]), colorVector, s.alpha);   // RT:699
                    counts[1]++;
                }
            }
            if (std::isnan(colorVector.X) || std::isnan(colorVector.Y) || std::isnan(colorVector.Z)) counts[2]++;
        } else {
            counts[3]++;
        }
        if (rgba_out) rgba_out[i] = ColorFromVector3(colorVector);   // RT:705
        if (rgb_f32_out) { rgb_f32_out[3 * i] = colorVector.X; rgb_f32_out[3 * i + 1] = colorVector.Y; rgb_f32_out[3 * i + 2] = colorVector.Z; }
    }
    if (counts_out) for (int k = 0; k < 4; k++) counts_out[k] = counts[k];
    return 0;
}

// RT:309 as the oracle's frames state it (oracle.cpp RayTracer::FixedSixteen / GetColorForQuadrant): samples == 4 the mean of four, 16 the mean of four means
int orc_fold_samples(const uint32_t *rgba_in, int64_t n, int32_t samples, uint32_t *rgba_out, float *rgb_f32_out) {
    if (samples != 4 && samples != 16) return -2;
    for (int64_t i = 0; i < n; i++) {
        uint32_t result;
        if (samples == 4) {
            const uint32_t *c = rgba_in + 4 * i;
            result = ColorFromVector3((ColorToVector3(c[0]) + ColorToVector3(c[1]) + ColorToVector3(c[2]) + ColorToVector3(c[3])) / 4.0f);
        } else {
            uint32_t corner[4];
            for (int q = 0; q < 4; q++) {
                const uint32_t *sub = rgba_in + 16 * i + 4 * q;
                corner[q] = ColorFromVector3((ColorToVector3(sub[0]) + ColorToVector3(sub[1]) + ColorToVector3(sub[2]) + ColorToVector3(sub[3])) / 4.0f);
            }
            result = ColorFromVector3((ColorToVector3(corner[0]) + ColorToVector3(corner[1]) + ColorToVector3(corner[2]) + ColorToVector3(corner[3])) / 4.0f);
        }
        rgba_out[i] = result;
        if (rgb_f32_out) { const Vector3 v = ColorToVector3(result); rgb_f32_out[3 * i] = v.X; rgb_f32_out[3 * i + 1] = v.Y; rgb_f32_out[3 * i + 2] = v.Z; }
    }
    return 0;
}

}  // extern "C"
