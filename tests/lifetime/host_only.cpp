// The lifetime of a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile `hostcheck`): create, one
// triangle, one body, build, save, load into a second scene, destroy both.  What it checks: every call returns XRT_OK, and that lifetime
// is clean on the host under AddressSanitizer, UBSan and LeakSanitizer.  Needs no GPU; prints "host_only: ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <unistd.h>

#include "../../include/xrt.h"

static int failed(const char *what, int rc) {
    fprintf(stderr, "host_only: %s returned %d: %s\n", what, rc, xrt_last_error());
    return 1;
}

int main() {
    if (xrt_version() != XRT_VERSION) return failed("xrt_version", xrt_version());
    const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, n[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1}, uv[6] = {0, 0, 1, 0, 0, 1}, sn[3] = {0, 0, 1};
    const float color[4] = {1, 0.5f, 0.25f, 1}, bbox[6] = {0, 0, 0, 1, 1, 0};
    const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.refraction_index = 1.0f;

    xrt_scene *a = nullptr, *b = nullptr;
    int32_t mesh = -1, body = -1;
    int rc;
    if ((rc = xrt_scene_create(-1, &a)) != XRT_OK) return failed("xrt_scene_create", rc);
    if ((rc = xrt_scene_add_mesh(a, v, n, uv, sn, color, 1, &mat, bbox, &mesh)) != XRT_OK) return failed("xrt_scene_add_mesh", rc);
    if ((rc = xrt_scene_add_object(a, &mesh, 1, ident, ident, bbox, bbox, &body)) != XRT_OK) return failed("xrt_scene_add_object", rc);
    if ((rc = xrt_scene_build(a, 0, 0)) != XRT_OK) return failed("xrt_scene_build", rc);

    char path[] = "/tmp/xrt_host_only_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { perror("host_only: mkstemp"); return 1; }
    close(fd);
    rc = xrt_scene_save(a, path);
    if (rc == XRT_OK) rc = xrt_scene_load(-1, path, &b);
    unlink(path);
    if (rc != XRT_OK) return failed("xrt_scene_save / xrt_scene_load", rc);
    if ((rc = xrt_scene_build(b, 0, 0)) != XRT_OK) return failed("xrt_scene_build (loaded scene)", rc);

    if ((rc = xrt_scene_destroy(a)) != XRT_OK) return failed("xrt_scene_destroy", rc);
    if ((rc = xrt_scene_destroy(b)) != XRT_OK) return failed("xrt_scene_destroy (loaded scene)", rc);
    printf("host_only: ok\n");
    return 0;
}
